// abi.hip -- the C ABI of libmatinv_hip.so: include/matinv.h (native, device-resident, stream-aware)
// and the 17 reference-named entry points of include/inverse_gpu.h in fp64 and (suffix _f32) fp32.
//
// No CPU fallback lives here: every entry point ends in a HIP kernel launch or fails loudly.
#include <errno.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "../../include/matinv.h"
#include "common.hpp"

using namespace matinv;

namespace {
thread_local char g_err[512] = "";
}

namespace matinv {
int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int fail_hip(hipError_t e, const char *what)
{
    return fail(MATINV_ERR_HIP, "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
}
}  // namespace matinv

namespace {

// The library is built for gfx950 only; refuse anything else instead of faulting in the launch.
int check_device()
{
    static thread_local int checked_dev = -1;
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail(MATINV_ERR_NO_DEVICE, "hipGetDevice: %s", hipGetErrorString(e));
    if (dev == checked_dev) return MATINV_OK;
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return fail_hip(e, "hipGetDeviceProperties");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MATINV_ERR_NO_DEVICE, "device %d is %s; libmatinv_hip is built for gfx950 (MI355X) only", dev,
                    prop.gcnArchName);
    checked_dev = dev;
    return MATINV_OK;
}

// Staging buffers of the host-pointer entry points: the library's scratch cache (scratch.hip), so that the reference-style
// "allocate, copy, run, copy, free inside every call" (batched_invert.cu:120-176) stops paying hipMalloc / hipFree (about 0.5 ms
// per call) after the first call.
hipError_t staging_alloc(void **p, size_t bytes) { return scratch_alloc(p, bytes, nullptr); }
void staging_free(void *p)
{
    if (p) (void)scratch_free(p, nullptr);
}

// One buffer of a host-pointer call: the caller's pointer (null: not staged) and its element count.
struct StagedIn {
    const void *host;
    size_t count;
};
struct StagedOut {
    void *host;
    size_t count;
};

// The host-pointer form of every family but gp_host and inverse_host*: allocate the non-null inputs in table order, then the non-null
// outputs, then info; copy the inputs in; call(din, dout, dInfo) -- the device pointers in table order, null where the table's host
// pointer is null -- which returns the rc of the family's dispatch; copy the outputs and info out when it succeeded; free everything.
// After a first HIP error nothing further is allocated, copied or launched. What a family stages under which request is decided
// by the pointers it puts into its tables alone.
template <class T, size_t NI, size_t NO, class Call>
int run_staged(const char *family, const StagedIn (&in)[NI], const StagedOut (&out)[NO], size_t batch, int *info, Call call)
{
    int rc = check_device();
    if (rc) return rc;
    T *din[NI] = {}, *dout[NO] = {};
    int *dInfo = nullptr;
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < NI && e == hipSuccess; ++i)
        if (in[i].host) e = staging_alloc(reinterpret_cast<void **>(&din[i]), in[i].count * sizeof(T));
    for (size_t i = 0; i < NO && e == hipSuccess; ++i)
        if (out[i].host) e = staging_alloc(reinterpret_cast<void **>(&dout[i]), out[i].count * sizeof(T));
    if (e == hipSuccess && info) e = staging_alloc(reinterpret_cast<void **>(&dInfo), batch * sizeof(int));
    for (size_t i = 0; i < NI && e == hipSuccess; ++i)
        if (din[i]) e = hipMemcpy(din[i], in[i].host, in[i].count * sizeof(T), hipMemcpyHostToDevice);
    if (e == hipSuccess) rc = call(din, dout, dInfo);
    for (size_t i = 0; i < NO && e == hipSuccess && rc == MATINV_OK; ++i)
        if (dout[i]) e = hipMemcpy(out[i].host, dout[i], out[i].count * sizeof(T), hipMemcpyDeviceToHost);
    if (e == hipSuccess && rc == MATINV_OK && info) e = hipMemcpy(info, dInfo, batch * sizeof(int), hipMemcpyDeviceToHost);
    for (T *p : din) staging_free(p);
    for (T *p : dout) staging_free(p);
    staging_free(dInfo);
    if (rc != MATINV_OK) return rc;
    if (e != hipSuccess) return fail_hip(e, (std::string(family) + " host<->device").c_str());
    return MATINV_OK;
}

// ---- the argument checks every family shares: one message each. A family's *_check_args reads: check_head, `if (batch == 0) return
// MATINV_OK;`, its own lines, check_tail, its own count limits. `name` is what the family calls its matrix order: "n" or "q". ---------
int check_order(const char *name, int n)
{
    if (n < 1) return fail(MATINV_ERR_ARG, "%s must be >= 1 (got %d)", name, n);
    return MATINV_OK;
}

int check_dtype(int dtype)
{
    if (dtype != MATINV_F64 && dtype != MATINV_F32) return fail(MATINV_ERR_ARG, "unknown dtype %d", dtype);
    return MATINV_OK;
}

// checked even for an empty batch
int check_head(const char *name, int n, int dtype)
{
    const int rc = check_order(name, n);
    return rc ? rc : check_dtype(dtype);
}

int check_batch(size_t batch)
{
    if (batch > 0x7fffffffu) return fail(MATINV_ERR_ARG, "batch %zu exceeds the grid limit; split the call", batch);
    return MATINV_OK;
}

// after the family's pointer and output checks: the grid limit, then the largest order any kernel family serves
int check_tail(const char *name, int n, size_t batch)
{
    const int rc = check_batch(batch);
    if (rc) return rc;
    if (n > 1024) return fail(MATINV_ERR_UNSUPPORTED, "%s=%d exceeds every kernel family built in (limit 1024)", name, n);
    return MATINV_OK;
}

// the per-call limit of a count (nquery, ntarget, nsample, npoint, nparam); `things` is what it counts
int check_count(const char *name, int count, const char *things)
{
    if (count > 1024) return fail(MATINV_ERR_UNSUPPORTED, "%s=%d exceeds the limit of 1024 %s per call", name, count, things);
    return MATINV_OK;
}

// The one dtype switch of the C ABI: f is a generic lambda, called with a value of the element type.
template <class F>
int by_dtype(int dtype, F f)
{
    if (dtype == MATINV_F64) return f(double());
    if (dtype == MATINV_F32) return f(float());
    return check_dtype(dtype);
}

// The guard of the GP families' matinv_*_kernel_name functions: they answer "" for an order or a dtype that no launch accepts.
bool has_kernel_name(int dtype, int n) { return n >= 1 && n <= 1024 && (dtype == MATINV_F64 || dtype == MATINV_F32); }

template <class T>
int select_auto(int algo, int n)
{
    if (algo == MATINV_ALGO_GAUSS_JORDAN) {
        if (rowlane_family_supports<T>(n)) return MATINV_KERNEL_ROWLANE;
        if (tile_family_supports<T>(n)) return MATINV_KERNEL_TILE;
        if (tileq_supports(sizeof(T) == 8, n)) return MATINV_KERNEL_TILEP;  // one wavefront per tile column, pivoting
        if (blocked_gj_supports(n)) return MATINV_KERNEL_BLOCKED;  // beyond n = 128 it beats the LDS kernel at every size measured
    } else if (rowlane_family_supports<T>(n)) {
        return MATINV_KERNEL_ROWLANE;  // several SPD matrices per wavefront
    } else if (spd_tile_supports<T>(n)) {
        return MATINV_KERNEL_TILE;
    } else if (blocked_inverse_supports(n)) {
        return MATINV_KERNEL_BLOCKED;  // SPD inverse beyond the four-wave kernel
    }
    if (lds_family_supports<T>(n)) return MATINV_KERNEL_LDS;
    if (global_family_supports<T>(n)) return MATINV_KERNEL_GLOBAL;
    return MATINV_ERR_UNSUPPORTED;
}

// Does the forced family `kernel` (not AUTO) have a kernel for a full inversion of size n? The launcher below and matinv_kernel_name both
// ask here, so a name is returned exactly where a launch would not be refused.
template <class T>
bool family_serves(int algo, int n, int kernel)
{
    const bool gj = algo == MATINV_ALGO_GAUSS_JORDAN;
    switch (kernel) {
    case MATINV_KERNEL_LDS: return lds_family_supports<T>(n);
    case MATINV_KERNEL_ROWLANE: return rowlane_family_supports<T>(n);
    case MATINV_KERNEL_TILE: return gj ? tile_family_supports<T>(n) : spd_tile_supports<T>(n);
    case MATINV_KERNEL_GLOBAL: return global_family_supports<T>(n);
    case MATINV_KERNEL_BLOCKED: return gj ? blocked_gj_supports(n) : blocked_inverse_supports(n);
    case MATINV_KERNEL_TILEP: return gj && (tilep_supports(n) || tileq_supports(sizeof(T) == 8, n));
    case MATINV_KERNEL_ROW: return gj && row_family_supports<T>(n);
    default: return false;
    }
}

template <class T>
int inverse_dispatch(int algo, int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *dInfo, hipStream_t stream,
                     int kernel, int chol_phases = 7)
{
    if (int rc = check_order("n", n)) return rc;
    if (algo != MATINV_ALGO_GAUSS_JORDAN && algo != MATINV_ALGO_CHOLESKY)
        return fail(MATINV_ERR_ARG, "unknown algorithm %d", algo);
    if (batch == 0) return MATINV_OK;
    int rc = check_batch(batch);
    if (rc == MATINV_OK) rc = check_device();
    if (rc) return rc;
    if (kernel == MATINV_KERNEL_AUTO) {
        // the Cholesky sub-phase entry points (factor only, ...) exist in the LDS family only
        kernel = (algo == MATINV_ALGO_CHOLESKY && chol_phases != 7 && lds_family_supports<T>(n)) ? (int)MATINV_KERNEL_LDS
                                                                                                 : select_auto<T>(algo, n);
        if (kernel < 0)
            return fail(MATINV_ERR_UNSUPPORTED, "n=%d exceeds every kernel family built in (limit 1024)", n);
    }
    hipError_t e = hipErrorInvalidValue;
    const bool serves = family_serves<T>(algo, n, kernel);
    switch (kernel) {
    case MATINV_KERNEL_LDS:
        if (!serves) return fail(MATINV_ERR_UNSUPPORTED, "LDS family: n=%d does not fit 160 KiB", n);
        e = (algo == MATINV_ALGO_GAUSS_JORDAN) ? launch_gj_lds<T>(n, A, X, batch, dInfo, stream)
                                               : launch_chol_lds<T>(n, A, X, batch, dInfo, stream, chol_phases);
        break;
    case MATINV_KERNEL_ROWLANE:
        if (!serves || (algo == MATINV_ALGO_CHOLESKY && chol_phases != 7))
            return fail(MATINV_ERR_UNSUPPORTED, "rowlane family serves full inversions with n <= 16 only (n=%d)", n);
        e = (algo == MATINV_ALGO_CHOLESKY) ? launch_spd_rowlane<T>(n, A, X, batch, dInfo, stream)
                                           : launch_gj_rowlane<T>(n, A, X, batch, dInfo, stream);
        break;
    case MATINV_KERNEL_TILE:
        if (algo == MATINV_ALGO_CHOLESKY) {
            if (!serves || chol_phases != 7)
                return fail(MATINV_ERR_UNSUPPORTED, "tile family serves the full SPD inverse with n <= 192 (f64) / 256 (f32) only (n=%d)", n);
            e = launch_spd_tile<T>(n, A, X, batch, dInfo, stream);
            break;
        }
        if (!serves)
            return fail(MATINV_ERR_UNSUPPORTED, "tile family serves Gauss-Jordan with n <= 192 (f64) / 256 (f32) only (n=%d)", n);
        e = launch_gj_tile<T>(n, A, X, batch, dInfo, stream);
        break;
    case MATINV_KERNEL_GLOBAL:
        if (!serves || chol_phases != 7)
            return fail(MATINV_ERR_UNSUPPORTED, "global family serves full inversions with n <= 1024 only (n=%d)", n);
        e = (algo == MATINV_ALGO_GAUSS_JORDAN) ? launch_gj_global<T>(n, A, X, batch, dInfo, stream)
                                               : launch_chol_global<T>(n, A, X, batch, dInfo, stream);
        break;
    case MATINV_KERNEL_BLOCKED:
        if (algo == MATINV_ALGO_GAUSS_JORDAN) {
            if (!serves) return fail(MATINV_ERR_UNSUPPORTED, "blocked family: n=%d exceeds the limit 1024", n);
            e = launch_gj_blocked<T>(n, A, X, batch, dInfo, stream);
            break;
        }
        if (!serves || chol_phases != 7)
            return fail(MATINV_ERR_UNSUPPORTED, "blocked family serves the full SPD inverse with n <= 1024 only (n=%d)", n);
        e = launch_chol_blocked<T>(n, A, X, batch, dInfo, stream);
        break;
    case MATINV_KERNEL_TILEP:
        if (!serves)
            return fail(MATINV_ERR_UNSUPPORTED, "pivoting tile family serves Gauss-Jordan with n <= 192 (f64) / 256 (f32) only (n=%d)", n);
        e = n > 128 ? launch_gj_tileq<T>(n, A, X, batch, dInfo, stream, nullptr, nullptr, nullptr, nullptr, nullptr)
                    : (n > 64 ? launch_gj_tilep4<T>(n, A, X, batch, dInfo, stream) : launch_gj_tilep<T>(n, A, X, batch, dInfo, stream));
        break;
    case MATINV_KERNEL_ROW:
        if (!serves)
            return fail(MATINV_ERR_UNSUPPORTED, "row family serves Gauss-Jordan with n <= 64 only (n=%d)", n);
        e = launch_gj_row<T>(n, A, X, batch, dInfo, stream);
        break;
    default:
        return fail(MATINV_ERR_ARG, "unknown kernel family %d", kernel);
    }
    if (e != hipSuccess) return fail_hip(e, "kernel launch");
    return MATINV_OK;
}

template <class T>
int inverse_strided(int algo, int n, const void *dA, size_t strideA, void *dAinv, size_t strideInv, size_t batch,
                    int *dInfo, void *stream, int kernel)
{
    if (int rc = check_order("n", n)) return rc;
    if (batch && (!dA || !dAinv)) return fail(MATINV_ERR_ARG, "null device pointer");
    if (batch > 1 && (strideA < (size_t)n * n || strideInv < (size_t)n * n))
        return fail(MATINV_ERR_ARG, "stride smaller than n*n");
    BatchRef<const T> A{static_cast<const T *>(dA), strideA, nullptr};
    BatchRef<T> X{static_cast<T *>(dAinv), strideInv, nullptr};
    return inverse_dispatch<T>(algo, n, A, X, batch, dInfo, static_cast<hipStream_t>(stream), kernel);
}

double now_ms()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

// MATINV_DETAILED_LOGGING=1 reproduces the reference's log=1 build (Makefile:115-117 there): one
// `name,batch,n,ms,ns\r\n` line per phase (include/timer.h:8-9), same key names as the reference's
// TIMER_LOG calls (e.g. src/gauss/batched_invert.cu:114-118,169-171).
bool detailed_logging()
{
    static int v = -1;
    if (v < 0) {
        const char *s = getenv("MATINV_DETAILED_LOGGING");
        v = (s && *s && *s != '0') ? 1 : 0;
    }
    return v == 1;
}

void timer_log(const char *prefix, const char *phase, size_t batch, int n, double ms)
{
    printf("%s_%s,%zu,%d,%.4f,%lu\r\n", prefix, phase, batch, n, ms, (unsigned long)(ms * 1e6));
}

// Large host batches: the caller's two buffers are page-locked in place (hipHostRegister) and the batch is cut into chunks
// that rotate over a few streams -- chunk i+1 uploads while chunk i is inverted and chunk i-1 downloads (PCIe is full
// duplex; the simple path below does H2D, kernel, D2H strictly one after the other, through the runtime's pageable
// staging). Device memory is chunk-sized, so a host batch larger than HBM also works.
// Returns MATINV_ERR_UNSUPPORTED (without touching the output) when the buffers cannot be registered; the caller then
// takes the simple path.
template <class T>
int inverse_host_pipelined(int algo, int n, const T *hA, T *hAinv, size_t batch, int *info, int kernel, double &ms_total,
                           bool registered = false)
{
    constexpr int NS = 3;  // streams / chunk slots in flight
    const size_t mat = (size_t)n * n, bytes_mat = mat * sizeof(T);
    size_t chunk = (size_t)(48u << 20) / bytes_mat;  // ~48 MiB per chunk
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    const double t0 = now_ms();
    if (!registered) {
        if (hipHostRegister(const_cast<T *>(hA), batch * bytes_mat, hipHostRegisterDefault) != hipSuccess) {
            (void)hipGetLastError();
            return MATINV_ERR_UNSUPPORTED;
        }
        if (hipHostRegister(hAinv, batch * bytes_mat, hipHostRegisterDefault) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipHostUnregister(const_cast<T *>(hA));
            return MATINV_ERR_UNSUPPORTED;
        }
    }
    hipStream_t st[NS] = {};
    T *dA[NS] = {}, *dX[NS] = {};
    int *dI[NS] = {};
    hipError_t e = hipSuccess;
    int rc = MATINV_OK;
    for (int s = 0; s < NS && e == hipSuccess; ++s) {
        e = hipStreamCreateWithFlags(&st[s], hipStreamNonBlocking);
        if (e == hipSuccess) e = scratch_alloc(reinterpret_cast<void **>(&dA[s]), chunk * bytes_mat, st[s]);
        if (e == hipSuccess) e = scratch_alloc(reinterpret_cast<void **>(&dX[s]), chunk * bytes_mat, st[s]);
        if (e == hipSuccess && info) e = scratch_alloc(reinterpret_cast<void **>(&dI[s]), chunk * sizeof(int), st[s]);
    }
    size_t slot = 0;
    for (size_t off = 0; off < batch && e == hipSuccess && rc == MATINV_OK; off += chunk, ++slot) {
        const int s = (int)(slot % NS);
        const size_t cnt = (batch - off < chunk) ? batch - off : chunk;
        // the slot's previous chunk has fully left the device once its stream is idle (same stream: in order anyway)
        e = hipMemcpyAsync(dA[s], hA + off * mat, cnt * bytes_mat, hipMemcpyHostToDevice, st[s]);
        if (e != hipSuccess) break;
        rc = inverse_strided<T>(algo, n, dA[s], mat, dX[s], mat, cnt, info ? dI[s] : nullptr, st[s], kernel);
        if (rc != MATINV_OK) break;
        e = hipMemcpyAsync(hAinv + off * mat, dX[s], cnt * bytes_mat, hipMemcpyDeviceToHost, st[s]);
        if (e == hipSuccess && info)
            e = hipMemcpyAsync(info + off, dI[s], cnt * sizeof(int), hipMemcpyDeviceToHost, st[s]);
    }
    for (int s = 0; s < NS; ++s) {
        if (st[s]) {
            hipError_t es = hipStreamSynchronize(st[s]);
            if (e == hipSuccess) e = es;
        }
        if (dA[s]) (void)scratch_free(dA[s], st[s]);
        if (dX[s]) (void)scratch_free(dX[s], st[s]);
        if (dI[s]) (void)scratch_free(dI[s], st[s]);
        if (st[s]) {
            scratch_retire_stream(st[s]);  // synchronised above: its blocks may serve any stream of this device from now on
            (void)hipStreamDestroy(st[s]);
        }
    }
    if (!registered) {
        (void)hipHostUnregister(const_cast<T *>(hA));
        (void)hipHostUnregister(hAinv);
    }
    ms_total = now_ms() - t0;
    if (rc != MATINV_OK) return rc;
    if (e != hipSuccess) return fail_hip(e, "pipelined host<->device transfer");
    return MATINV_OK;
}

template <class T>
int inverse_host_multi(int algo, int n, const void *hA, void *hAinv, size_t batch, int *info, int nshards, int kernel);

// MATINV_DEVICES=N (> 1): the host-pointer entry points shard over N devices (matinv_inverse_batched_host_multi)
int env_devices()
{
    static const int v = []() {
        const char *s = getenv("MATINV_DEVICES");
        return s && *s ? atoi(s) : 0;
    }();
    return v;
}

// host_mode (set by the multi-device driver for its per-shard calls): HOST_REGISTERED = both host buffers are page-locked for every
// device already; HOST_STAGED_ONLY = its up-front page-locking failed -- go straight to the staged copies (a per-shard
// hipHostRegister would collide with the neighbours' on shared pages: ADVICE r03)
enum { HOST_DEFAULT = 0, HOST_REGISTERED = 1, HOST_STAGED_ONLY = 2 };
template <class T>
int inverse_host(int algo, int n, const void *hA, void *hAinv, size_t batch, int *info, const char *log_prefix,
                 int kernel = MATINV_KERNEL_AUTO, bool single_device = false, int host_mode = HOST_DEFAULT)
{
    const bool registered = host_mode == HOST_REGISTERED;
    if (n < 1) return fail(MATINV_ERR_ARG, "n must be >= 1 (got %d)", n);
    if (batch == 0) return MATINV_OK;
    if (!hA || !hAinv) return fail(MATINV_ERR_ARG, "null host pointer");
    if (!single_device && env_devices() > 1) {
        const double t0 = now_ms();
        const int mrc = inverse_host_multi<T>(algo, n, hA, hAinv, batch, info, env_devices(), kernel);
        // MATINV_DEVICES > 1 under MATINV_DETAILED_LOGGING: one line for the whole sharded call (the shards overlap: no phase split)
        if (mrc == MATINV_OK && detailed_logging() && log_prefix) timer_log(log_prefix, "multi_total", batch, n, now_ms() - t0);
        return mrc;
    }
    int rc = check_device();
    if (rc) return rc;
    const size_t elems = (size_t)n * n * batch;  // size_t: 1M x 64 x 64 overflows the reference's int index
    {
        // pipelined path for batches worth it (>= 128 MiB per direction); MATINV_HOST_PIPELINE=0/1 forces it off/on
        static const int mode = []() {
            const char *s = getenv("MATINV_HOST_PIPELINE");
            return s && *s ? atoi(s) : -1;
        }();
        const bool big = elems * sizeof(T) >= ((size_t)128 << 20);
        if (hA != hAinv && host_mode != HOST_STAGED_ONLY && (registered || mode == 1 || (mode < 0 && big))) {
            double ms = 0;
            const int prc = inverse_host_pipelined<T>(algo, n, static_cast<const T *>(hA), static_cast<T *>(hAinv), batch, info,
                                                      kernel, ms, registered);
            if (prc != MATINV_ERR_UNSUPPORTED) {
                if (prc == MATINV_OK && detailed_logging() && log_prefix) timer_log(log_prefix, "pipelined_total", batch, n, ms);
                return prc;
            }
        }
    }
    T *dA = nullptr, *dX = nullptr;
    int *dInfo = nullptr;
    hipError_t e;
    const bool log = detailed_logging() && log_prefix;
    if ((e = staging_alloc(reinterpret_cast<void **>(&dA), elems * sizeof(T))) != hipSuccess) return fail_hip(e, "hipMalloc(As)");
    if ((e = staging_alloc(reinterpret_cast<void **>(&dX), elems * sizeof(T))) != hipSuccess) {
        staging_free(dA);
        return fail_hip(e, "hipMalloc(aInvs)");
    }
    if (info && (e = staging_alloc(reinterpret_cast<void **>(&dInfo), batch * sizeof(int))) != hipSuccess) {
        staging_free(dA);
        staging_free(dX);
        return fail_hip(e, "hipMalloc(info)");
    }
    double t0 = now_ms();
    e = hipMemcpy(dA, hA, elems * sizeof(T), hipMemcpyHostToDevice);
    double t1 = now_ms();
    if (e == hipSuccess) {
        rc = inverse_strided<T>(algo, n, dA, (size_t)n * n, dX, (size_t)n * n, batch, dInfo, nullptr, kernel);
        if (rc == MATINV_OK && log) e = hipDeviceSynchronize();
    }
    double t2 = now_ms();
    if (e == hipSuccess && rc == MATINV_OK) e = hipMemcpy(hAinv, dX, elems * sizeof(T), hipMemcpyDeviceToHost);
    if (e == hipSuccess && rc == MATINV_OK && info)
        e = hipMemcpy(info, dInfo, batch * sizeof(int), hipMemcpyDeviceToHost);
    double t3 = now_ms();
    staging_free(dA);
    staging_free(dX);
    staging_free(dInfo);
    if (rc != MATINV_OK) return rc;
    if (e != hipSuccess) return fail_hip(e, "host<->device copy");
    if (log) {
        timer_log(log_prefix, "mem_htod", batch, n, t1 - t0);
        timer_log(log_prefix, "ker", batch, n, t2 - t1);
        timer_log(log_prefix, "mem_dtoh", batch, n, t3 - t2);
    }
    return MATINV_OK;
}

// contiguous block partition of [0, batch): ceil(batch / nshards) per shard, rounded up to the per-wavefront packing factor of the
// small-n kernels (8 matrices per wave for n <= 8, 4 for n <= 16) so that no wavefront straddles two shards; trailing shards may be
// short or empty (shard.partition in Python)
void shard_range(size_t batch, int nshards, int n, int g, size_t &lo, size_t &hi)
{
    const size_t mult = n <= 8 ? 8 : (n <= 16 ? 4 : 1);
    size_t per = (batch + (size_t)nshards - 1) / (size_t)nshards;
    per = (per + mult - 1) / mult * mult;
    lo = std::min(batch, (size_t)g * per);
    hi = std::min(batch, lo + per);
}

int gfx950_devices(std::vector<int> &devs)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess) return fail(MATINV_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    for (int d = 0; d < count; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) devs.push_back(d);
    }
    if (devs.empty()) return fail(MATINV_ERR_NO_DEVICE, "no gfx950 (MI355X) device visible");
    return MATINV_OK;
}

// The batch over several devices of this process: contiguous blocks (the partition of shard.py / SURVEY 8e: ceil(batch /
// nshards) rounded up to the per-wavefront packing factor), one host thread per shard with hipSetDevice, each running the
// single-device host path on its slice -- the pipelined one (upload, kernel and download of 48 MiB chunks rotating over three
// streams) over its own host link when the slices are large. Nothing is exchanged between devices: results go back to host
// memory. Shards beyond the device count share devices round robin ("virtual shards": what a one-GPU box can test).
template <class T>
int inverse_host_multi(int algo, int n, const void *hA, void *hAinv, size_t batch, int *info, int nshards, int kernel)
{
    if (n < 1) return fail(MATINV_ERR_ARG, "n must be >= 1 (got %d)", n);
    if (batch == 0) return MATINV_OK;
    if (!hA || !hAinv) return fail(MATINV_ERR_ARG, "null host pointer");
    std::vector<int> devs;
    int rc = gfx950_devices(devs);
    if (rc) return rc;
    if (nshards <= 0) nshards = (int)devs.size();
    if (nshards > 1024) return fail(MATINV_ERR_ARG, "nshards %d: at most 1024", nshards);
    const size_t mat = (size_t)n * n;
    int home = 0;
    (void)hipGetDevice(&home);
    // page-lock both buffers ONCE for every device (adjacent shards share pages: per-shard registration would collide);
    // small batches and aliasing buffers go through the plain staged copies instead
    const bool pin = hA != hAinv && batch * mat * sizeof(T) >= ((size_t)64 << 20);
    bool pinned = false;
    if (pin) {
        if (hipHostRegister(const_cast<void *>(hA), batch * mat * sizeof(T), hipHostRegisterPortable) == hipSuccess) {
            if (hipHostRegister(hAinv, batch * mat * sizeof(T), hipHostRegisterPortable) == hipSuccess) pinned = true;
            else (void)hipHostUnregister(const_cast<void *>(hA));
        }
        if (!pinned) (void)hipGetLastError();
    }
    struct Result {
        int rc = MATINV_OK;
        std::string msg;
    };
    std::vector<Result> res((size_t)nshards);
    std::vector<std::thread> workers;
    for (int g = 0; g < nshards; ++g) {
        size_t lo = 0, hi = 0;
        shard_range(batch, nshards, n, g, lo, hi);
        if (hi == lo) continue;
        const int dev = devs[(size_t)g % devs.size()];
        workers.emplace_back([=, &res]() {
            hipError_t e = hipSetDevice(dev);
            int r = e == hipSuccess ? inverse_host<T>(algo, n, static_cast<const T *>(hA) + lo * mat, static_cast<T *>(hAinv) + lo * mat,
                                                      hi - lo, info ? info + lo : nullptr, nullptr, kernel, true,
                                                      pinned ? HOST_REGISTERED : (pin ? HOST_STAGED_ONLY : HOST_DEFAULT))
                                    : fail_hip(e, "hipSetDevice");
            res[(size_t)g].rc = r;
            if (r != MATINV_OK) res[(size_t)g].msg = g_err;  // the worker's thread-local message
        });
    }
    for (auto &t : workers) t.join();
    if (pinned) {
        (void)hipHostUnregister(const_cast<void *>(hA));
        (void)hipHostUnregister(hAinv);
    }
    (void)hipSetDevice(home);
    for (int g = 0; g < nshards; ++g)
        if (res[(size_t)g].rc != MATINV_OK) return fail(res[(size_t)g].rc, "shard %d of %d: %s", g, nshards, res[(size_t)g].msg.c_str());
    return MATINV_OK;
}

// Reference *_batched_device form: HOST-resident tables of DEVICE pointers (filled by batchedCudaMalloc,
// /root/reference/src/helper.cu:103-118, so normally equally spaced by the pitch). Equally spaced tables are
// passed as base + stride; anything else is staged into a device-side table that lives until the launch retires.
template <class T>
int inverse_table(int algo, int n, T *const *hostIn, T *const *hostOut, size_t batch, int chol_phases = 7,
                  int kernel = MATINV_KERNEL_AUTO)
{
    if (int rc = check_order("n", n)) return rc;
    if (batch == 0) return MATINV_OK;
    if (!hostIn || !hostOut) return fail(MATINV_ERR_ARG, "null pointer table");
    auto uniform = [&](T *const *tab, size_t &stride) {
        stride = (size_t)n * n;
        if (batch == 1) return true;
        if (tab[1] <= tab[0]) return false;
        stride = (size_t)(tab[1] - tab[0]);
        if (stride < (size_t)n * n) return false;
        for (size_t i = 2; i < batch; ++i)
            if (tab[i] != tab[0] + i * stride) return false;
        return true;
    };
    size_t sIn = 0, sOut = 0;
    const bool uIn = uniform(hostIn, sIn), uOut = uniform(hostOut, sOut);
    T **dTabIn = nullptr, **dTabOut = nullptr;
    hipError_t e = hipSuccess;
    if (!uIn) {
        if ((e = hipMalloc(&dTabIn, batch * sizeof(T *))) != hipSuccess) return fail_hip(e, "hipMalloc(table)");
        e = hipMemcpy(dTabIn, hostIn, batch * sizeof(T *), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && !uOut) {
        if ((e = hipMalloc(&dTabOut, batch * sizeof(T *))) == hipSuccess)
            e = hipMemcpy(dTabOut, hostOut, batch * sizeof(T *), hipMemcpyHostToDevice);
    }
    int rc = MATINV_OK;
    if (e != hipSuccess) rc = fail_hip(e, "pointer table staging");
    if (rc == MATINV_OK) {
        BatchRef<const T> A{hostIn[0], sIn, uIn ? nullptr : const_cast<const T *const *>(dTabIn)};
        BatchRef<T> X{hostOut[0], sOut, uOut ? nullptr : dTabOut};
        rc = inverse_dispatch<T>(algo, n, A, X, batch, nullptr, nullptr, kernel, chol_phases);
    }
    if (dTabIn || dTabOut) {
        // rare path: the table must outlive the asynchronous launch
        (void)hipDeviceSynchronize();
        if (dTabIn) (void)hipFree(dTabIn);
        if (dTabOut) (void)hipFree(dTabOut);
    }
    return rc;
}

// ---- batched linear solve X = A^-1 B (matinv_solve_batched) ------------------------------------------------------------------
// Which path a solve request takes: the fused bordered tile kernel (or, under MATINV_GJ_PIVOT, the row solve) for 16 < n <= 64 and
// nrhs <= 16; otherwise the composed path (inverse of `family` into a scratch block, then the batched product).
enum { SOLVE_FUSED = 0, SOLVE_ROW = 1, SOLVE_COMPOSED = 2 };
int solve_route(int algo, int n, int nrhs, int kernel, int &family)
{
    family = MATINV_KERNEL_AUTO;
    const bool fused = solve_tile_supports(n, nrhs);
    if (kernel == MATINV_KERNEL_TILE) {
        if (!fused)
            return fail(MATINV_ERR_UNSUPPORTED, "the fused solve serves 16 < n <= 64 and nrhs <= 16 only (n=%d, nrhs=%d)", n, nrhs);
        return SOLVE_FUSED;
    }
    if (kernel == MATINV_KERNEL_AUTO && fused)
        return (algo == MATINV_ALGO_GAUSS_JORDAN && gj_policy() == MATINV_GJ_PIVOT) ? SOLVE_ROW : SOLVE_FUSED;
    family = kernel;
    return SOLVE_COMPOSED;
}

int solve_check_args(int algo, int dtype, int n, int nrhs, const void *dA, size_t strideA, const void *dB, size_t strideB, void *dX,
                     size_t strideX, size_t batch, int kernel)
{
    if (int rc = check_order("n", n)) return rc;
    if (nrhs < 1) return fail(MATINV_ERR_ARG, "nrhs must be >= 1 (got %d)", nrhs);
    if (algo != MATINV_ALGO_GAUSS_JORDAN && algo != MATINV_ALGO_CHOLESKY) return fail(MATINV_ERR_ARG, "unknown algorithm %d", algo);
    if (int rc = check_dtype(dtype)) return rc;
    if (kernel < MATINV_KERNEL_AUTO || kernel > MATINV_KERNEL_TILEP) return fail(MATINV_ERR_ARG, "unknown kernel family %d", kernel);
    if (batch == 0) return MATINV_OK;
    if (!dA || !dB || !dX) return fail(MATINV_ERR_ARG, "null device pointer");
    const size_t nb = (size_t)n * (size_t)nrhs;
    if (batch > 1 && (strideA < (size_t)n * n || strideB < nb || strideX < nb))
        return fail(MATINV_ERR_ARG, "stride too small (strideA >= n*n, strideB and strideX >= n*nrhs)");
    return check_tail("n", n, batch);
}

template <class T>
int solve_strided(int algo, int n, int nrhs, const void *dA, size_t strideA, const void *dB, size_t strideB, void *dX, size_t strideX,
                  size_t batch, int *dInfo, hipStream_t stream, int kernel)
{
    int family = MATINV_KERNEL_AUTO;
    const int route = solve_route(algo, n, nrhs, kernel, family);
    if (route < 0) return route;
    int rc = check_device();
    if (rc) return rc;
    BatchRef<const T> A{static_cast<const T *>(dA), strideA, nullptr};
    BatchRef<const T> B{static_cast<const T *>(dB), strideB, nullptr};
    BatchRef<T> X{static_cast<T *>(dX), strideX, nullptr};
    hipError_t e = hipSuccess;
    if (route == SOLVE_FUSED) {
        e = launch_solve_tile<T>(algo, n, nrhs, A, B, X, batch, dInfo, stream);
    } else if (route == SOLVE_ROW) {
        e = launch_solve_row<T>(n, nrhs, A, B, X, batch, dInfo, stream);
    } else {
        // composed: k-range chunks whose inverses fit the blocked-path workspace cap, each inverted by the forced (or automatic)
        // family into scratch -- its own info and NaN contract -- then X = Ainv B
        const size_t mat = (size_t)n * n;
        size_t chunk = blocked_workspace_cap() / (mat * sizeof(T));
        if (chunk < 1) chunk = 1;
        if (chunk > batch) chunk = batch;
        T *inv = nullptr;
        e = scratch_alloc(reinterpret_cast<void **>(&inv), chunk * mat * sizeof(T), stream);
        if (e != hipSuccess) return fail_hip(e, "solve workspace");
        for (size_t off = 0; off < batch && rc == MATINV_OK && e == hipSuccess; off += chunk) {
            const size_t cnt = batch - off < chunk ? batch - off : chunk;
            BatchRef<const T> Ac{A.base + off * strideA, strideA, nullptr};
            BatchRef<T> Inv{inv, mat, nullptr};
            rc = inverse_dispatch<T>(algo, n, Ac, Inv, cnt, dInfo ? dInfo + off : nullptr, stream, family);
            if (rc == MATINV_OK)
                e = launch_solve_gemm<T>(n, nrhs, inv, BatchRef<const T>{B.base + off * strideB, strideB, nullptr},
                                         BatchRef<T>{X.base + off * strideX, strideX, nullptr}, cnt, stream);
        }
        const hipError_t e2 = scratch_free(inv, stream);
        if (rc != MATINV_OK) return rc;
        if (e == hipSuccess) e = e2;
    }
    if (e != hipSuccess) return fail_hip(e, "solve launch");
    return MATINV_OK;
}

template <class T>
int solve_host(int algo, int n, int nrhs, const void *hA, const void *hB, void *hX, size_t batch, int *info)
{
    const size_t ea = (size_t)n * n * batch, eb = (size_t)n * nrhs * batch;
    const StagedIn in[] = {{hA, ea}, {hB, eb}};
    const StagedOut out[] = {{hX, eb}};
    return run_staged<T>("solve", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return solve_strided<T>(algo, n, nrhs, i[0], (size_t)n * n, i[1], (size_t)n * nrhs, o[0], (size_t)n * nrhs, batch, dInfo, nullptr,
                                MATINV_KERNEL_AUTO);
    });
}

// Which kernel a fused mean / variance request takes (the name function and the launcher both ask here):
//   n <= 16 the rowlane kernel; 16 < n <= 25 the two-rows-per-lane kernel, inverse folded in registers;
//   then the MFMA tile kernels, one to three wavefronts per item, lower tiles only: fp64 112 < n <= 176 on two wavefronts, 176 < n <= 192 on
//   three (spd_tile2_impl.hpp), the SPD sweep with the bilinear form folded out of the accumulators where the bordered form no longer fits
//   one wavefront (fp64 80 < n <= 112, fp32 96 < n <= 160), the bordered sweep below that;
//   beyond the tile kernels (fp64 n > 192, fp32 n > 160) the blocked Cholesky path, up to n = 1024.
enum { GP_ROWLANE = 0, GP_ROWLANE2, GP_SPD_TILE2, GP_SPD_TILE, GP_TILE, GP_BLOCKED };
template <class T>
int gp_route(int n)
{
    constexpr bool f64 = sizeof(T) == 8;
    if (rowlane_family_supports<T>(n)) return GP_ROWLANE;
    if (rowlane2_supports(n)) return GP_ROWLANE2;
    if (f64 && spd_tile2_supports(true, n)) return GP_SPD_TILE2;
    if (gp_spd_tile_supports(f64, n)) return GP_SPD_TILE;
    if (gp_tile_supports(f64, n)) return GP_TILE;
    if (!global_family_supports<T>(n)) return fail(MATINV_ERR_UNSUPPORTED, "pipeline: n=%d exceeds the limit 1024", n);
    return GP_BLOCKED;
}

template <class T>
int gp_dispatch(int n, const void *a, const void *B, const void *c, const void *d, const void *e_, void *out,
                size_t batch, int *dInfo, void *stream, bool variance)
{
    if (int rc = check_order("n", n)) return rc;
    if (batch == 0) return MATINV_OK;
    if (!a || !B || !c || !out || (variance ? !e_ : !d)) return fail(MATINV_ERR_ARG, "null device pointer");
    int rc = check_batch(batch);
    if (rc == MATINV_OK) rc = check_device();
    if (rc) return rc;
    const int route = gp_route<T>(n);
    if (route < 0) return route;
    const T *As = static_cast<const T *>(a), *Bs = static_cast<const T *>(B), *Cs = static_cast<const T *>(c);
    const T *Ds = variance ? nullptr : static_cast<const T *>(d), *Es = static_cast<const T *>(e_);
    T *o = static_cast<T *>(out);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipErrorInvalidValue;
    switch (route) {
    case GP_ROWLANE: e = launch_gp_rowlane<T>(n, As, Bs, Cs, Ds, Es, o, batch, dInfo, st); break;
    case GP_ROWLANE2: e = launch_gp_rowlane2<T>(n, As, Bs, Cs, Ds, Es, o, batch, dInfo, st); break;
    case GP_SPD_TILE2:
        if constexpr (sizeof(T) == 8) e = launch_gp_spd_tile2(n, As, Bs, Cs, Ds, Es, o, batch, dInfo, st);
        break;
    case GP_SPD_TILE: e = launch_gp_spd_tile<T>(n, As, Bs, Cs, Ds, Es, o, batch, dInfo, st); break;
    case GP_TILE: e = launch_gp_tile<T>(n, As, Bs, Cs, Ds, Es, o, batch, dInfo, st); break;
    case GP_BLOCKED: e = launch_gp_blocked<T>(n, As, Bs, Cs, Ds, Es, o, batch, dInfo, st); break;
    }
    if (e != hipSuccess) return fail_hip(e, "kernel launch");
    return MATINV_OK;
}

// Host-pointer form of the fused pipeline (what gauss_bench's calcluateMean / calcluateVariance time,
// /root/reference/src/gauss_bench.cu:127-265): allocate, H2D, one kernel, D2H of batch scalars, free.
template <class T>
int gp_host(int n, const void *hA, const void *hB, const void *hC, const void *hX, void *hOut, size_t batch, int *info,
            bool variance)
{
    if (n < 1) return fail(MATINV_ERR_ARG, "n must be >= 1 (got %d)", n);
    if (batch == 0) return MATINV_OK;
    if (!hA || !hB || !hC || !hX || !hOut) return fail(MATINV_ERR_ARG, "null host pointer");
    int rc = check_device();
    if (rc) return rc;
    const size_t vec = (size_t)n * batch, mat = vec * n, xlen = variance ? batch : vec;
    const bool log = detailed_logging();
    const char *key = variance ? "calculate_variance_gpu" : "calculate_mean_gpu";
    T *dA = nullptr, *dB = nullptr, *dC = nullptr, *dX = nullptr, *dOut = nullptr;
    int *dInfo = nullptr;
    hipError_t e = hipSuccess;
    auto alloc = [&](T **p, size_t count) {
        if (e == hipSuccess) e = staging_alloc(reinterpret_cast<void **>(p), count * sizeof(T));
    };
    alloc(&dA, vec), alloc(&dB, mat), alloc(&dC, vec), alloc(&dX, xlen), alloc(&dOut, batch);
    if (e == hipSuccess && info) e = staging_alloc(reinterpret_cast<void **>(&dInfo), batch * sizeof(int));
    const double t0 = now_ms();
    auto h2d = [&](T *d, const void *h, size_t count) {
        if (e == hipSuccess) e = hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice);
    };
    h2d(dA, hA, vec), h2d(dB, hB, mat), h2d(dC, hC, vec), h2d(dX, hX, xlen);
    const double t1 = now_ms();
    if (e == hipSuccess) {
        rc = gp_dispatch<T>(n, dA, dB, dC, variance ? nullptr : dX, variance ? dX : nullptr, dOut, batch, dInfo, nullptr,
                            variance);
        if (rc == MATINV_OK && log) e = hipDeviceSynchronize();
    }
    const double t2 = now_ms();
    if (e == hipSuccess && rc == MATINV_OK) e = hipMemcpy(hOut, dOut, batch * sizeof(T), hipMemcpyDeviceToHost);
    if (e == hipSuccess && rc == MATINV_OK && info) e = hipMemcpy(info, dInfo, batch * sizeof(int), hipMemcpyDeviceToHost);
    const double t3 = now_ms();
    staging_free(dA), staging_free(dB), staging_free(dC), staging_free(dX), staging_free(dOut);
    staging_free(dInfo);
    if (rc != MATINV_OK) return rc;
    if (e != hipSuccess) return fail_hip(e, "pipeline host<->device");
    if (log) {
        // the reference's six keys (src/gauss_bench.cu:151-156,250-255; results/generate_plots.m:69-76 sums them): the
        // fused kernel does add + inv + mul + dot in one launch, so its time is booked under _inv and the others are 0
        timer_log(key, "mem_htod", batch, n, t1 - t0);
        timer_log(key, "add", batch, n, 0.0);
        timer_log(key, "inv", batch, n, t2 - t1);
        timer_log(key, "mul", batch, n, 0.0);
        timer_log(key, "dot", batch, n, 0.0);
        timer_log(key, "mem_dtoh", batch, n, t3 - t2);
    }
    return MATINV_OK;
}

// ---- batched log-determinant and GP log marginal likelihood (matinv_logdet_batched, matinv_logml_batched) --------------------------
// Which kernel a logdet request takes: the MFMA tile sweep (Cholesky, n <= 96), the pivoting row kernel (Gauss-Jordan, n <= 64),
// the global-memory kernel for everything else up to n = 1024.
enum { LOGDET_TILE = 0, LOGDET_ROW = 1, LOGDET_GLOBAL = 2 };
int logdet_route(int algo, int n, int kernel)
{
    const bool tile = algo == MATINV_ALGO_CHOLESKY && logdet_tile_supports(n);
    const bool row = algo == MATINV_ALGO_GAUSS_JORDAN && logdet_row_supports(n);
    switch (kernel) {
    case MATINV_KERNEL_AUTO: return tile ? LOGDET_TILE : row ? LOGDET_ROW : LOGDET_GLOBAL;
    case MATINV_KERNEL_TILE:
        if (!tile) return fail(MATINV_ERR_UNSUPPORTED, "the logdet tile kernel serves MATINV_ALGO_CHOLESKY with n <= 96 only (n=%d)", n);
        return LOGDET_TILE;
    case MATINV_KERNEL_ROW:
        if (!row) return fail(MATINV_ERR_UNSUPPORTED, "the logdet row kernel serves MATINV_ALGO_GAUSS_JORDAN with n <= 64 only (n=%d)", n);
        return LOGDET_ROW;
    case MATINV_KERNEL_GLOBAL: return LOGDET_GLOBAL;
    default: return fail(MATINV_ERR_UNSUPPORTED, "kernel family %d has no logdet kernel (TILE, ROW, GLOBAL)", kernel);
    }
}

int logdet_check_args(int algo, int dtype, int n, const void *dA, size_t strideA, const void *dLogAbsDet, size_t batch, int kernel)
{
    if (int rc = check_order("n", n)) return rc;
    if (algo != MATINV_ALGO_GAUSS_JORDAN && algo != MATINV_ALGO_CHOLESKY) return fail(MATINV_ERR_ARG, "unknown algorithm %d", algo);
    if (int rc = check_dtype(dtype)) return rc;
    if (kernel < MATINV_KERNEL_AUTO || kernel > MATINV_KERNEL_TILEP) return fail(MATINV_ERR_ARG, "unknown kernel family %d", kernel);
    if (batch == 0) return MATINV_OK;
    if (!dA || !dLogAbsDet) return fail(MATINV_ERR_ARG, "null device pointer");
    if (batch > 1 && strideA < (size_t)n * n) return fail(MATINV_ERR_ARG, "stride too small (strideA >= n*n)");
    return check_tail("n", n, batch);
}

template <class T>
int logdet_strided(int algo, int n, const void *dA, size_t strideA, void *dLogAbsDet, void *dSign, size_t batch, int *dInfo,
                   hipStream_t stream, int kernel)
{
    const int route = logdet_route(algo, n, kernel);
    if (route < 0) return route;
    int rc = check_device();
    if (rc) return rc;
    const T *A = static_cast<const T *>(dA);
    T *ld = static_cast<T *>(dLogAbsDet), *sg = static_cast<T *>(dSign);
    hipError_t e;
    if (route == LOGDET_TILE) e = launch_logdet_tile<T>(n, false, A, strideA, nullptr, nullptr, ld, sg, batch, dInfo, stream);
    else if (route == LOGDET_ROW) e = launch_logdet_row<T>(n, A, strideA, ld, sg, batch, dInfo, stream);
    else e = launch_logdet_global<T>(n, algo == MATINV_ALGO_CHOLESKY, A, strideA, nullptr, ld, sg, batch, dInfo, stream);
    if (e != hipSuccess) return fail_hip(e, "logdet launch");
    return MATINV_OK;
}

template <class T>
int logdet_host(int algo, int n, const void *hA, void *hLogAbsDet, void *hSign, size_t batch, int *info)
{
    const StagedIn in[] = {{hA, (size_t)n * n * batch}};
    const StagedOut out[] = {{hLogAbsDet, batch}, {hSign, batch}};
    return run_staged<T>("logdet", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return logdet_strided<T>(algo, n, i[0], (size_t)n * n, o[0], o[1], batch, dInfo, nullptr, MATINV_KERNEL_AUTO);
    });
}

int logml_check_args(int dtype, int n, const void *dBs, const void *dDs, const void *dLogml, size_t batch)
{
    if (int rc = check_head("n", n, dtype)) return rc;
    if (batch == 0) return MATINV_OK;
    if (!dBs || !dDs || !dLogml) return fail(MATINV_ERR_ARG, "null device pointer");
    return check_tail("n", n, batch);
}

// n <= 96: the bordered tile kernel. Beyond: the variance pipeline with a = d and e = 0 puts -d^T M^-1 d into scratch, the global
// logdet kernel with diag = c the determinant (and info), a small kernel combines them.
enum { LOGML_TILE = 0, LOGML_COMPOSED = 1 };
int logml_route(int n) { return logdet_tile_supports(n) ? LOGML_TILE : LOGML_COMPOSED; }

template <class T>
int logml_dispatch(int n, const void *dBs, const void *dCs, const void *dDs, void *dLogml, size_t batch, int *dInfo, hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *B = static_cast<const T *>(dBs), *c = static_cast<const T *>(dCs), *d = static_cast<const T *>(dDs);
    T *out = static_cast<T *>(dLogml);
    switch (logml_route(n)) {
    case LOGML_TILE: {
        const hipError_t e = launch_logdet_tile<T>(n, true, B, (size_t)n * n, c, d, out, nullptr, batch, dInfo, stream);
        if (e != hipSuccess) return fail_hip(e, "logml launch");
        return MATINV_OK;
    }
    default: break;
    }
    // scratch: [e = 0 | (c = 0 when absent)] [var] [logdet]
    const size_t zeros = batch + (c ? 0 : batch * (size_t)n);
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), (zeros + 2 * batch) * sizeof(T), stream);
    if (e != hipSuccess) return fail_hip(e, "logml workspace");
    T *zero_e = ws, *var = ws + zeros, *ld = var + batch;
    const T *cc = c ? c : ws + batch;
    e = hipMemsetAsync(ws, 0, zeros * sizeof(T), stream);
    if (e == hipSuccess) rc = gp_dispatch<T>(n, d, B, cc, nullptr, zero_e, var, batch, nullptr, stream, true);
    if (e == hipSuccess && rc == MATINV_OK) e = launch_logdet_global<T>(n, true, B, (size_t)n * n, c, ld, nullptr, batch, dInfo, stream);
    if (e == hipSuccess && rc == MATINV_OK) e = launch_logml_combine<T>(n, var, ld, out, batch, stream);
    const hipError_t e2 = scratch_free(ws, stream);
    if (rc != MATINV_OK) return rc;
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail_hip(e, "logml launch");
    return MATINV_OK;
}

template <class T>
int logml_host(int n, const void *hBs, const void *hCs, const void *hDs, void *hLogml, size_t batch, int *info)
{
    const size_t vec = (size_t)n * batch, mat = vec * n;
    const StagedIn in[] = {{hBs, mat}, {hCs, vec}, {hDs, vec}};
    const StagedOut out[] = {{hLogml, batch}};
    return run_staged<T>("logml", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return logml_dispatch<T>(n, i[0], i[1], i[2], o[0], batch, dInfo, nullptr);
    });
}

// ---- batched leave-one-out cross-validation of a GP (matinv_loo_batched) ---------------------------------------------------------------
int loo_check_args(int dtype, int n, const void *dBs, const void *dDs, const void *dMean, const void *dVar, const void *dLogPL, size_t batch)
{
    if (int rc = check_head("n", n, dtype)) return rc;
    if (batch == 0) return MATINV_OK;
    if (!dBs || !dDs) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!dMean && !dVar && !dLogPL) return fail(MATINV_ERR_ARG, "no output requested (mean, var and logpl are all null)");
    return check_tail("n", n, batch);
}

// n <= 96: the LOO form of the one-wavefront SPD sweep. Beyond, to n = 1024: the LOO form of the global-memory Cholesky kernel.
template <class T>
int loo_dispatch(int n, const void *dBs, const void *dCs, const void *dDs, void *dMean, void *dVar, void *dLogPL, size_t batch, int *dInfo,
                 hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *B = static_cast<const T *>(dBs), *c = static_cast<const T *>(dCs), *d = static_cast<const T *>(dDs);
    T *mean = static_cast<T *>(dMean), *var = static_cast<T *>(dVar), *logpl = static_cast<T *>(dLogPL);
    const hipError_t e = loo_tile_supports(n) ? launch_loo_tile<T>(n, B, c, d, mean, var, logpl, batch, dInfo, stream)
                                              : launch_loo_global<T>(n, B, c, d, mean, var, logpl, batch, dInfo, stream);
    if (e != hipSuccess) return fail_hip(e, "loo launch");
    return MATINV_OK;
}

template <class T>
int loo_host(int n, const void *hBs, const void *hCs, const void *hDs, void *hMean, void *hVar, void *hLogPL, size_t batch, int *info)
{
    const size_t vec = (size_t)n * batch, mat = vec * n;
    const StagedIn in[] = {{hBs, mat}, {hCs, vec}, {hDs, vec}};
    const StagedOut out[] = {{hMean, vec}, {hVar, vec}, {hLogPL, batch}};
    return run_staged<T>("loo", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return loo_dispatch<T>(n, i[0], i[1], i[2], o[0], o[1], o[2], batch, dInfo, nullptr);
    });
}

// ---- gradients of the batched GP log marginal likelihood (matinv_logml_grad_batched) -------------------------------------------------
int logml_grad_check_args(int dtype, int n, int nparam, const void *dBs, const void *dDs, const void *dDMs, const void *dGrad,
                          const void *dGradC, const void *dAlpha, size_t batch)
{
    if (int rc = check_head("n", n, dtype)) return rc;
    if (batch == 0) return MATINV_OK;
    if (nparam < 0) return fail(MATINV_ERR_ARG, "nparam must be >= 0 (got %d)", nparam);
    if (!dBs || !dDs) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!dGrad && !dGradC && !dAlpha) return fail(MATINV_ERR_ARG, "no output requested (grad, gradc and alpha are all null)");
    if (dGrad && nparam < 1) return fail(MATINV_ERR_ARG, "grad requested with nparam = 0");
    if (dGrad && !dDMs) return fail(MATINV_ERR_ARG, "grad requested without derivative matrices (dDMs is null)");
    return check_tail("n", n, batch);
}

// n <= 96: the gradient form of the one-wavefront SPD sweep. Beyond, to n = 1024: the gradient form of the global-memory Cholesky kernel.
template <class T>
int logml_grad_dispatch(int n, int nparam, const void *dBs, const void *dCs, const void *dDs, const void *dDMs, void *dGrad, void *dGradC,
                        void *dAlpha, size_t batch, int *dInfo, hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *B = static_cast<const T *>(dBs), *c = static_cast<const T *>(dCs), *d = static_cast<const T *>(dDs);
    const T *dM = static_cast<const T *>(dDMs);
    T *grad = static_cast<T *>(dGrad), *gradc = static_cast<T *>(dGradC), *alpha = static_cast<T *>(dAlpha);
    const hipError_t e = logml_grad_tile_supports(n)
                             ? launch_logml_grad_tile<T>(n, nparam, B, c, d, dM, grad, gradc, alpha, batch, dInfo, stream)
                             : launch_logml_grad_global<T>(n, nparam, B, c, d, dM, grad, gradc, alpha, batch, dInfo, stream);
    if (e != hipSuccess) return fail_hip(e, "logml_grad launch");
    return MATINV_OK;
}

template <class T>
int logml_grad_host(int n, int nparam, const void *hBs, const void *hCs, const void *hDs, const void *hDMs, void *hGrad, void *hGradC,
                    void *hAlpha, size_t batch, int *info)
{
    const size_t vec = (size_t)n * batch, mat = vec * n, par = batch * (size_t)nparam;
    // the derivative matrices are read for grad only
    const StagedIn in[] = {{hBs, mat}, {hCs, vec}, {hDs, vec}, {hGrad ? hDMs : nullptr, par * (size_t)n * n}};
    const StagedOut out[] = {{hGrad, par}, {hGradC, vec}, {hAlpha, vec}};
    return run_staged<T>("logml_grad", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return logml_grad_dispatch<T>(n, nparam, i[0], i[1], i[2], i[3], o[0], o[1], o[2], batch, dInfo, nullptr);
    });
}

// ---- gradients of the batched GP leave-one-out log pseudo-likelihood (matinv_loo_grad_batched) -----------------------------------------
int loo_grad_check_args(int dtype, int n, int nparam, const void *dBs, const void *dDs, const void *dDMs, const void *dGrad,
                        const void *dGradC, const void *dLogPL, size_t batch)
{
    if (int rc = check_head("n", n, dtype)) return rc;
    if (batch == 0) return MATINV_OK;
    if (nparam < 0) return fail(MATINV_ERR_ARG, "nparam must be >= 0 (got %d)", nparam);
    if (!dBs || !dDs) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!dGrad && !dGradC && !dLogPL) return fail(MATINV_ERR_ARG, "no output requested (grad, gradc and logpl are all null)");
    if (dGrad && nparam < 1) return fail(MATINV_ERR_ARG, "grad requested with nparam = 0");
    if (dGrad && !dDMs) return fail(MATINV_ERR_ARG, "grad requested without derivative matrices (dDMs is null)");
    return check_tail("n", n, batch);
}

// n <= 96: the LOO-gradient form of the one-wavefront SPD sweep. Beyond, to n = 1024: that of the global-memory Cholesky kernel.
template <class T>
int loo_grad_dispatch(int n, int nparam, const void *dBs, const void *dCs, const void *dDs, const void *dDMs, void *dGrad, void *dGradC,
                      void *dLogPL, size_t batch, int *dInfo, hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *B = static_cast<const T *>(dBs), *c = static_cast<const T *>(dCs), *d = static_cast<const T *>(dDs);
    const T *dM = static_cast<const T *>(dDMs);
    T *grad = static_cast<T *>(dGrad), *gradc = static_cast<T *>(dGradC), *logpl = static_cast<T *>(dLogPL);
    const hipError_t e = loo_grad_tile_supports(n)
                             ? launch_loo_grad_tile<T>(n, nparam, B, c, d, dM, grad, gradc, logpl, batch, dInfo, stream)
                             : launch_loo_grad_global<T>(n, nparam, B, c, d, dM, grad, gradc, logpl, batch, dInfo, stream);
    if (e != hipSuccess) return fail_hip(e, "loo_grad launch");
    return MATINV_OK;
}

template <class T>
int loo_grad_host(int n, int nparam, const void *hBs, const void *hCs, const void *hDs, const void *hDMs, void *hGrad, void *hGradC,
                  void *hLogPL, size_t batch, int *info)
{
    const size_t vec = (size_t)n * batch, mat = vec * n, par = batch * (size_t)nparam;
    // the derivative matrices are read for grad only
    const StagedIn in[] = {{hBs, mat}, {hCs, vec}, {hDs, vec}, {hGrad ? hDMs : nullptr, par * (size_t)n * n}};
    const StagedOut out[] = {{hGrad, par}, {hGradC, vec}, {hLogPL, batch}};
    return run_staged<T>("loo_grad", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return loo_grad_dispatch<T>(n, nparam, i[0], i[1], i[2], i[3], o[0], o[1], o[2], batch, dInfo, nullptr);
    });
}

// ---- batched GP prediction at many query points per matrix (matinv_predict_batched) ---------------------------------------------------
int predict_check_args(int dtype, int n, int nquery, const void *dBs, const void *dDs, const void *dAs, const void *dMean, const void *dVar,
                       size_t batch)
{
    if (int rc = check_head("n", n, dtype)) return rc;
    if (batch == 0) return MATINV_OK;
    if (nquery < 1) return fail(MATINV_ERR_ARG, "nquery must be >= 1 (got %d)", nquery);
    if (!dBs || !dAs) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!dMean && !dVar) return fail(MATINV_ERR_ARG, "no output requested (mean and var are both null)");
    if (dMean && !dDs) return fail(MATINV_ERR_ARG, "mean requested without the observations (dDs is null)");
    return check_tail("n", n, batch);
}

// n <= 96: the prediction form of the one-wavefront SPD sweep. Beyond, to n = 1024: the prediction form of the global-memory Cholesky kernel.
template <class T>
int predict_dispatch(int n, int nquery, const void *dBs, const void *dCs, const void *dDs, const void *dAs, const void *dEs, void *dMean,
                     void *dVar, size_t batch, int *dInfo, hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *B = static_cast<const T *>(dBs), *c = static_cast<const T *>(dCs), *d = static_cast<const T *>(dDs);
    const T *a = static_cast<const T *>(dAs), *e_ = static_cast<const T *>(dEs);
    T *mean = static_cast<T *>(dMean), *var = static_cast<T *>(dVar);
    const hipError_t e = predict_tile_supports(n) ? launch_predict_tile<T>(n, nquery, B, c, d, a, e_, mean, var, batch, dInfo, stream)
                                                  : launch_predict_global<T>(n, nquery, B, c, d, a, e_, mean, var, batch, dInfo, stream);
    if (e != hipSuccess) return fail_hip(e, "predict launch");
    return MATINV_OK;
}

template <class T>
int predict_host(int n, int nquery, const void *hBs, const void *hCs, const void *hDs, const void *hAs, const void *hEs, void *hMean,
                 void *hVar, size_t batch, int *info)
{
    const size_t vec = (size_t)n * batch, mat = vec * n, qs = batch * (size_t)nquery;
    // the observations are read for mean only, the prior variances for var only
    const StagedIn in[] = {{hBs, mat}, {hCs, vec}, {hMean ? hDs : nullptr, vec}, {hAs, qs * (size_t)n}, {hVar ? hEs : nullptr, qs}};
    const StagedOut out[] = {{hMean, qs}, {hVar, qs}};
    return run_staged<T>("predict", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return predict_dispatch<T>(n, nquery, i[0], i[1], i[2], i[3], i[4], o[0], o[1], batch, dInfo, nullptr);
    });
}

// ---- batched joint predictive covariance between the query points of a matrix (matinv_predict_cov_batched) ----------------------------
int predict_cov_check_args(int dtype, int n, int nquery, const void *dBs, const void *dDs, const void *dAs, const void *dMean,
                           const void *dCov, size_t batch)
{
    if (int rc = check_head("n", n, dtype)) return rc;
    if (batch == 0) return MATINV_OK;
    if (nquery < 1) return fail(MATINV_ERR_ARG, "nquery must be >= 1 (got %d)", nquery);
    if (!dBs || !dAs) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!dMean && !dCov) return fail(MATINV_ERR_ARG, "no output requested (mean and cov are both null)");
    if (dMean && !dDs) return fail(MATINV_ERR_ARG, "mean requested without the observations (dDs is null)");
    if (int rc = check_tail("n", n, batch)) return rc;
    return check_count("nquery", nquery, "query points");
}

// n <= 96: the covariance form of the one-wavefront SPD sweep. Beyond, to n = 1024: the covariance form of the global-memory Cholesky kernel.
template <class T>
int predict_cov_dispatch(int n, int nquery, const void *dBs, const void *dCs, const void *dDs, const void *dAs, const void *dEs, void *dMean,
                         void *dCov, size_t batch, int *dInfo, hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *B = static_cast<const T *>(dBs), *c = static_cast<const T *>(dCs), *d = static_cast<const T *>(dDs);
    const T *a = static_cast<const T *>(dAs), *e_ = static_cast<const T *>(dEs);
    T *mean = static_cast<T *>(dMean), *cov = static_cast<T *>(dCov);
    const hipError_t e = predict_cov_tile_supports(n)
                             ? launch_predict_cov_tile<T>(n, nquery, B, c, d, a, e_, mean, cov, batch, dInfo, stream)
                             : launch_predict_cov_global<T>(n, nquery, B, c, d, a, e_, mean, cov, batch, dInfo, stream);
    if (e != hipSuccess) return fail_hip(e, "predict_cov launch");
    return MATINV_OK;
}

template <class T>
int predict_cov_host(int n, int nquery, const void *hBs, const void *hCs, const void *hDs, const void *hAs, const void *hEs, void *hMean,
                     void *hCov, size_t batch, int *info)
{
    const size_t vec = (size_t)n * batch, mat = vec * n, qs = batch * (size_t)nquery, qq = qs * (size_t)nquery;
    // the observations are read for mean only, the prior covariances for cov only
    const StagedIn in[] = {{hBs, mat}, {hCs, vec}, {hMean ? hDs : nullptr, vec}, {hAs, qs * (size_t)n}, {hCov ? hEs : nullptr, qq}};
    const StagedOut out[] = {{hMean, qs}, {hCov, qq}};
    return run_staged<T>("predict_cov", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return predict_cov_dispatch<T>(n, nquery, i[0], i[1], i[2], i[3], i[4], o[0], o[1], batch, dInfo, nullptr);
    });
}

// ---- batched Cholesky factor and coloured samples Y = m + chol(C) Z (matinv_colour_batched) ---------------------------------------------
int colour_check_args(int dtype, int q, int nsample, const void *dC, size_t strideC, const void *dZ, const void *dY, const void *dL,
                      size_t batch)
{
    if (int rc = check_head("q", q, dtype)) return rc;
    if (batch == 0) return MATINV_OK;
    if (!dC) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!dY && !dL) return fail(MATINV_ERR_ARG, "no output requested (Y and L are both null)");
    if (dY && !dZ) return fail(MATINV_ERR_ARG, "Y requested without the samples (dZ is null)");
    if (dY && nsample < 1) return fail(MATINV_ERR_ARG, "nsample must be >= 1 with Y (got %d)", nsample);
    if (strideC < (size_t)q * q) return fail(MATINV_ERR_ARG, "strideC %zu is smaller than q*q", strideC);
    int rc = check_tail("q", q, batch);
    if (rc == MATINV_OK && dY) rc = check_count("nsample", nsample, "samples");
    return rc;
}

// q <= 96: the colour form of the one-wavefront SPD sweep. Beyond, to q = 1024: the colour form of the global-memory Cholesky kernel.
// info_base: see launch_colour_tile (common.hpp).
template <class T>
int colour_dispatch(int q, int nsample, const void *dC, size_t strideC, const void *dM, const void *dZ, void *dY, void *dL, size_t batch,
                    int *dInfo, int info_base, hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *C = static_cast<const T *>(dC), *m = static_cast<const T *>(dM), *z = static_cast<const T *>(dZ);
    T *Y = static_cast<T *>(dY), *L = static_cast<T *>(dL);
    const hipError_t e = colour_tile_supports(q) ? launch_colour_tile<T>(q, nsample, C, strideC, m, z, Y, L, batch, dInfo, info_base, stream)
                                                 : launch_colour_global<T>(q, nsample, C, strideC, m, z, Y, L, batch, dInfo, info_base, stream);
    if (e != hipSuccess) return fail_hip(e, "colour launch");
    return MATINV_OK;
}

template <class T>
int colour_host(int q, int nsample, const void *hC, size_t strideC, const void *hM, const void *hZ, void *hY, void *hL, size_t batch,
                int *info)
{
    const size_t vec = (size_t)q * batch, mat = vec * q, ys = hY ? vec * (size_t)nsample : 0, cs = (batch - 1) * strideC + (size_t)q * q;
    // the mean and the samples are read for Y only
    const StagedIn in[] = {{hC, cs}, {hY ? hM : nullptr, vec}, {hY ? hZ : nullptr, ys}};
    const StagedOut out[] = {{hY, ys}, {hL, mat}};
    return run_staged<T>("colour", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return colour_dispatch<T>(q, nsample, i[0], strideC, i[1], i[2], o[0], o[1], batch, dInfo, 0, nullptr);
    });
}

// ---- batched whitening W = chol(C)^-1 (X - m), Mahalanobis distances and Gaussian log-density (matinv_whiten_batched) ------------------
// the checks of colour_check_args, in its order
int whiten_check_args(int dtype, int q, int npoint, const void *dC, size_t strideC, const void *dX, const void *dW, const void *dMaha,
                      const void *dLogdet, const void *dLogpdf, size_t batch)
{
    const bool points = dW || dMaha || dLogpdf;
    if (int rc = check_head("q", q, dtype)) return rc;
    if (batch == 0) return MATINV_OK;
    if (!dC) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!points && !dLogdet) return fail(MATINV_ERR_ARG, "no output requested (W, maha, logdet and logpdf are all null)");
    if (points && !dX) return fail(MATINV_ERR_ARG, "W, maha or logpdf requested without the points (dX is null)");
    if (points && npoint < 1) return fail(MATINV_ERR_ARG, "npoint must be >= 1 with W, maha or logpdf (got %d)", npoint);
    if (strideC < (size_t)q * q) return fail(MATINV_ERR_ARG, "strideC %zu is smaller than q*q", strideC);
    int rc = check_tail("q", q, batch);
    if (rc == MATINV_OK && points) rc = check_count("npoint", npoint, "points");
    return rc;
}

// q <= 96: the whiten form of the one-wavefront SPD sweep. Beyond, to q = 1024: the whiten form of the global-memory Cholesky kernel.
template <class T>
int whiten_dispatch(int q, int npoint, const void *dC, size_t strideC, const void *dM, const void *dX, void *dW, void *dMaha, void *dLogdet,
                    void *dLogpdf, size_t batch, int *dInfo, hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *C = static_cast<const T *>(dC), *m = static_cast<const T *>(dM), *x = static_cast<const T *>(dX);
    T *W = static_cast<T *>(dW), *mh = static_cast<T *>(dMaha), *ld = static_cast<T *>(dLogdet), *lp = static_cast<T *>(dLogpdf);
    const hipError_t e = whiten_tile_supports(q) ? launch_whiten_tile<T>(q, npoint, C, strideC, m, x, W, mh, ld, lp, batch, dInfo, stream)
                                                 : launch_whiten_global<T>(q, npoint, C, strideC, m, x, W, mh, ld, lp, batch, dInfo, stream);
    if (e != hipSuccess) return fail_hip(e, "whiten launch");
    return MATINV_OK;
}

template <class T>
int whiten_host(int q, int npoint, const void *hC, size_t strideC, const void *hM, const void *hX, void *hW, void *hMaha, void *hLogdet,
                void *hLogpdf, size_t batch, int *info)
{
    const bool points = hW || hMaha || hLogpdf;
    const size_t vec = (size_t)q * batch, ps = points ? batch * (size_t)npoint : 0, xs = vec * (points ? (size_t)npoint : 0);
    const size_t cs = (batch - 1) * strideC + (size_t)q * q;
    // the mean and the points are read for the per-point outputs only
    const StagedIn in[] = {{hC, cs}, {points ? hM : nullptr, vec}, {points ? hX : nullptr, xs}};
    const StagedOut out[] = {{hW, xs}, {hMaha, ps}, {hLogdet, batch}, {hLogpdf, ps}};
    return run_staged<T>("whiten", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return whiten_dispatch<T>(q, npoint, i[0], strideC, i[1], i[2], o[0], o[1], o[2], o[3], batch, dInfo, nullptr);
    });
}

// ---- batched multi-output GP solves: many target vectors per covariance matrix (matinv_multi_target_batched) ---------------------------
// the checks of predict_check_args, in its order
int multi_target_check_args(int dtype, int n, int ntarget, int nquery, const void *dBs, const void *dYs, const void *dAs, const void *dAlpha,
                            const void *dQuad, const void *dLogdet, const void *dLogml, const void *dMean, size_t batch)
{
    const bool targets = dAlpha || dQuad || dLogml || dMean;
    if (int rc = check_head("n", n, dtype)) return rc;
    if (batch == 0) return MATINV_OK;
    if (targets && ntarget < 1) return fail(MATINV_ERR_ARG, "ntarget must be >= 1 with alpha, quad, logml or mean (got %d)", ntarget);
    if (dMean && nquery < 1) return fail(MATINV_ERR_ARG, "nquery must be >= 1 with mean (got %d)", nquery);
    if (!dBs) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!targets && !dLogdet) return fail(MATINV_ERR_ARG, "no output requested (alpha, quad, logdet, logml and mean are all null)");
    if (targets && !dYs) return fail(MATINV_ERR_ARG, "alpha, quad, logml or mean requested without the targets (dYs is null)");
    if (dMean && !dAs) return fail(MATINV_ERR_ARG, "mean requested without the query vectors (dAs is null)");
    int rc = check_tail("n", n, batch);
    if (rc == MATINV_OK && targets) rc = check_count("ntarget", ntarget, "targets");
    if (rc == MATINV_OK && dMean) rc = check_count("nquery", nquery, "query points");
    return rc;
}

// n <= 96: the multi-target form of the one-wavefront SPD sweep. Beyond, to n = 1024: that of the global-memory Cholesky kernel.
template <class T>
int multi_target_dispatch(int n, int ntarget, int nquery, const void *dBs, const void *dCs, const void *dYs, const void *dAs, void *dAlpha,
                          void *dQuad, void *dLogdet, void *dLogml, void *dMean, size_t batch, int *dInfo, hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *B = static_cast<const T *>(dBs), *c = static_cast<const T *>(dCs), *y = static_cast<const T *>(dYs);
    const T *a = static_cast<const T *>(dAs);
    T *al = static_cast<T *>(dAlpha), *qd = static_cast<T *>(dQuad), *ld = static_cast<T *>(dLogdet), *lm = static_cast<T *>(dLogml);
    T *mn = static_cast<T *>(dMean);
    const hipError_t e = multi_target_tile_supports(n)
                             ? launch_multi_target_tile<T>(n, ntarget, nquery, B, c, y, a, al, qd, ld, lm, mn, batch, dInfo, stream)
                             : launch_multi_target_global<T>(n, ntarget, nquery, B, c, y, a, al, qd, ld, lm, mn, batch, dInfo, stream);
    if (e != hipSuccess) return fail_hip(e, "multi_target launch");
    return MATINV_OK;
}

template <class T>
int multi_target_host(int n, int ntarget, int nquery, const void *hBs, const void *hCs, const void *hYs, const void *hAs, void *hAlpha,
                      void *hQuad, void *hLogdet, void *hLogml, void *hMean, size_t batch, int *info)
{
    const bool targets = hAlpha || hQuad || hLogml || hMean;
    const size_t vec = (size_t)n * batch, mat = vec * n, ts = targets ? batch * (size_t)ntarget : 0, ys = ts * n;
    const size_t qs = hMean ? batch * (size_t)nquery : 0, ms = hMean ? ts * (size_t)nquery : 0;
    // the targets are read for every output but logdet, the query vectors for mean only
    const StagedIn in[] = {{hBs, mat}, {hCs, vec}, {targets ? hYs : nullptr, ys}, {hMean ? hAs : nullptr, qs * (size_t)n}};
    const StagedOut out[] = {{hAlpha, ys}, {hQuad, ts}, {hLogdet, batch}, {hLogml, ts}, {hMean, ms}};
    return run_staged<T>("multi_target", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return multi_target_dispatch<T>(n, ntarget, nquery, i[0], i[1], i[2], i[3], o[0], o[1], o[2], o[3], o[4], batch, dInfo, nullptr);
    });
}

// ---- gradients of the multi-output GP log marginal likelihood (matinv_multi_target_grad_batched) ---------------------------------------
// the checks of multi_target_check_args, in its order; every output needs the targets
int multi_target_grad_check_args(int dtype, int n, int ntarget, int nparam, const void *dBs, const void *dYs, const void *dDMs,
                                 const void *dGrad, const void *dGradC, const void *dLogml, const void *dAlpha, size_t batch)
{
    if (int rc = check_head("n", n, dtype)) return rc;
    if (batch == 0) return MATINV_OK;
    if (ntarget < 1) return fail(MATINV_ERR_ARG, "ntarget must be >= 1 (got %d)", ntarget);
    if (nparam < 0 || (dGrad && nparam < 1)) return fail(MATINV_ERR_ARG, "nparam must be >= 1 with grad, >= 0 without (got %d)", nparam);
    if (!dBs) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!dGrad && !dGradC && !dLogml && !dAlpha) return fail(MATINV_ERR_ARG, "no output requested (grad, gradc, logml and alpha are all null)");
    if (!dYs) return fail(MATINV_ERR_ARG, "the targets are needed for every output (dYs is null)");
    if (dGrad && !dDMs) return fail(MATINV_ERR_ARG, "grad requested without derivative matrices (dDMs is null)");
    int rc = check_tail("n", n, batch);
    if (rc == MATINV_OK) rc = check_count("ntarget", ntarget, "targets");
    if (rc == MATINV_OK && dGrad) rc = check_count("nparam", nparam, "derivative matrices");
    return rc;
}

// n <= 96: the gradient form of the multi-target tile kernels. Beyond, to n = 1024: that of the global-memory Cholesky kernel.
template <class T>
int multi_target_grad_dispatch(int n, int ntarget, int nparam, const void *dBs, const void *dCs, const void *dYs, const void *dDMs,
                               void *dGrad, void *dGradC, void *dLogml, void *dAlpha, size_t batch, int *dInfo, hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *B = static_cast<const T *>(dBs), *c = static_cast<const T *>(dCs), *y = static_cast<const T *>(dYs);
    const T *dM = dGrad ? static_cast<const T *>(dDMs) : nullptr;  // not read without grad
    T *grad = static_cast<T *>(dGrad), *gradc = static_cast<T *>(dGradC), *lm = static_cast<T *>(dLogml), *al = static_cast<T *>(dAlpha);
    const hipError_t e =
        multi_target_grad_tile_supports(n)
            ? launch_multi_target_grad_tile<T>(n, ntarget, nparam, B, c, y, dM, grad, gradc, lm, al, batch, dInfo, stream)
            : launch_multi_target_grad_global<T>(n, ntarget, nparam, B, c, y, dM, grad, gradc, lm, al, batch, dInfo, stream);
    if (e != hipSuccess) return fail_hip(e, "multi_target_grad launch");
    return MATINV_OK;
}

template <class T>
int multi_target_grad_host(int n, int ntarget, int nparam, const void *hBs, const void *hCs, const void *hYs, const void *hDMs, void *hGrad,
                           void *hGradC, void *hLogml, void *hAlpha, size_t batch, int *info)
{
    const size_t vec = (size_t)n * batch, mat = vec * n, ts = batch * (size_t)ntarget, ys = ts * n;
    const size_t par = hGrad ? batch * (size_t)nparam : 0;
    // the derivative matrices are read for grad only
    const StagedIn in[] = {{hBs, mat}, {hCs, vec}, {hYs, ys}, {hGrad ? hDMs : nullptr, par * (size_t)n * n}};
    const StagedOut out[] = {{hGrad, par}, {hGradC, vec}, {hLogml, ts}, {hAlpha, ys}};
    return run_staged<T>("multi_target_grad", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return multi_target_grad_dispatch<T>(n, ntarget, nparam, i[0], i[1], i[2], i[3], o[0], o[1], o[2], o[3], batch, dInfo, nullptr);
    });
}

// ---- batched GP regression with a linear trend (matinv_trend_batched) --------------------------------------------------------------------
// the checks of multi_target_check_args, in its order; the basis count is checked with n and dtype, before the empty batch returns
int trend_check_args(int dtype, int n, int nbasis, int ntarget, int nquery, const void *dBs, const void *dHs, const void *dYs, const void *dAs,
                     const void *dGs, const void *dEs, const void *dBeta, const void *dCovBeta, const void *dAlpha, const void *dQuad,
                     const void *dLogml, const void *dMean, const void *dVar, size_t batch)
{
    const bool targets = dBeta || dAlpha || dQuad || dLogml || dMean, queries = dMean || dVar;
    if (int rc = check_head("n", n, dtype)) return rc;
    if (nbasis < 1 || nbasis > 16) return fail(MATINV_ERR_ARG, "nbasis must be in 1 .. 16 (got %d)", nbasis);
    if (nbasis > n) return fail(MATINV_ERR_ARG, "nbasis=%d exceeds n=%d: H^T M^-1 H would be singular", nbasis, n);
    if (batch == 0) return MATINV_OK;
    if (targets && ntarget < 1) return fail(MATINV_ERR_ARG, "ntarget must be >= 1 with beta, alpha, quad, logml or mean (got %d)", ntarget);
    if (queries && nquery < 1) return fail(MATINV_ERR_ARG, "nquery must be >= 1 with mean or var (got %d)", nquery);
    if (!dBs || !dHs) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!targets && !dCovBeta && !dVar)
        return fail(MATINV_ERR_ARG, "no output requested (beta, covbeta, alpha, quad, logml, mean and var are all null)");
    if (targets && !dYs) return fail(MATINV_ERR_ARG, "beta, alpha, quad, logml or mean requested without the targets (dYs is null)");
    if (queries && !dAs) return fail(MATINV_ERR_ARG, "mean or var requested without the query vectors (dAs is null)");
    if (queries && !dGs) return fail(MATINV_ERR_ARG, "mean or var requested without the basis values of the queries (dGs is null)");
    if (dVar && !dEs) return fail(MATINV_ERR_ARG, "var requested without the prior variances (dEs is null)");
    int rc = check_tail("n", n, batch);
    if (rc == MATINV_OK && targets) rc = check_count("ntarget", ntarget, "targets");
    if (rc == MATINV_OK && queries) rc = check_count("nquery", nquery, "query points");
    return rc;
}

// n <= 96: the trend form of the one-wavefront SPD sweep. Beyond, to n = 1024: that of the global-memory Cholesky kernel.
template <class T>
int trend_dispatch(int n, int nbasis, int ntarget, int nquery, const void *dBs, const void *dCs, const void *dHs, const void *dYs,
                   const void *dAs, const void *dGs, const void *dEs, void *dBeta, void *dCovBeta, void *dAlpha, void *dQuad, void *dLogml,
                   void *dMean, void *dVar, size_t batch, int *dInfo, hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *B = static_cast<const T *>(dBs), *c = static_cast<const T *>(dCs), *h = static_cast<const T *>(dHs);
    const T *y = static_cast<const T *>(dYs), *a = static_cast<const T *>(dAs), *g = static_cast<const T *>(dGs);
    const T *e0 = static_cast<const T *>(dEs);
    T *be = static_cast<T *>(dBeta), *cb = static_cast<T *>(dCovBeta), *al = static_cast<T *>(dAlpha), *qd = static_cast<T *>(dQuad);
    T *lm = static_cast<T *>(dLogml), *mn = static_cast<T *>(dMean), *vr = static_cast<T *>(dVar);
    const hipError_t e =
        trend_tile_supports(n)
            ? launch_trend_tile<T>(n, nbasis, ntarget, nquery, B, c, h, y, a, g, e0, be, cb, al, qd, lm, mn, vr, batch, dInfo, stream)
            : launch_trend_global<T>(n, nbasis, ntarget, nquery, B, c, h, y, a, g, e0, be, cb, al, qd, lm, mn, vr, batch, dInfo, stream);
    if (e != hipSuccess) return fail_hip(e, "trend launch");
    return MATINV_OK;
}

template <class T>
int trend_host(int n, int nbasis, int ntarget, int nquery, const void *hBs, const void *hCs, const void *hHs, const void *hYs,
               const void *hAs, const void *hGs, const void *hEs, void *hBeta, void *hCovBeta, void *hAlpha, void *hQuad, void *hLogml,
               void *hMean, void *hVar, size_t batch, int *info)
{
    const bool targets = hBeta || hAlpha || hQuad || hLogml || hMean, queries = hMean || hVar;
    const size_t K = (size_t)nbasis, vec = (size_t)n * batch, mat = vec * n, ts = targets ? batch * (size_t)ntarget : 0;
    const size_t qs = queries ? batch * (size_t)nquery : 0;
    // the targets are read for beta, alpha, quad, logml and mean, the query vectors and their basis values for mean and var, the prior
    // variances for var only
    const StagedIn in[] = {{hBs, mat},
                           {hCs, vec},
                           {hHs, vec * K},
                           {targets ? hYs : nullptr, ts * n},
                           {queries ? hAs : nullptr, qs * n},
                           {queries ? hGs : nullptr, qs * K},
                           {hVar ? hEs : nullptr, qs}};
    const StagedOut out[] = {{hBeta, ts * K}, {hCovBeta, batch * K * K}, {hAlpha, ts * n}, {hQuad, ts}, {hLogml, ts},
                             {hMean, ts * (size_t)nquery}, {hVar, qs}};
    return run_staged<T>("trend", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return trend_dispatch<T>(n, nbasis, ntarget, nquery, i[0], i[1], i[2], i[3], i[4], i[5], i[6], o[0], o[1], o[2], o[3], o[4], o[5],
                                 o[6], batch, dInfo, nullptr);
    });
}

// ---- gradients of the restricted log marginal likelihood of the trend model (matinv_trend_grad_batched) ----------------------------------
// the checks of trend_check_args, in its order, with the lines of multi_target_grad_check_args for nparam and dDMs; every output needs the
// targets
int trend_grad_check_args(int dtype, int n, int nbasis, int ntarget, int nparam, const void *dBs, const void *dHs, const void *dYs,
                          const void *dDMs, const void *dGrad, const void *dGradC, const void *dLogml, const void *dAlpha, const void *dBeta,
                          size_t batch)
{
    if (int rc = check_head("n", n, dtype)) return rc;
    if (nbasis < 1 || nbasis > 16) return fail(MATINV_ERR_ARG, "nbasis must be in 1 .. 16 (got %d)", nbasis);
    if (nbasis > n) return fail(MATINV_ERR_ARG, "nbasis=%d exceeds n=%d: H^T M^-1 H would be singular", nbasis, n);
    if (batch == 0) return MATINV_OK;
    if (ntarget < 1) return fail(MATINV_ERR_ARG, "ntarget must be >= 1 (got %d)", ntarget);
    if (nparam < 0 || (dGrad && nparam < 1)) return fail(MATINV_ERR_ARG, "nparam must be >= 1 with grad, >= 0 without (got %d)", nparam);
    if (!dBs || !dHs) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!dGrad && !dGradC && !dLogml && !dAlpha && !dBeta)
        return fail(MATINV_ERR_ARG, "no output requested (grad, gradc, logml, alpha and beta are all null)");
    if (!dYs) return fail(MATINV_ERR_ARG, "the targets are needed for every output (dYs is null)");
    if (dGrad && !dDMs) return fail(MATINV_ERR_ARG, "grad requested without derivative matrices (dDMs is null)");
    int rc = check_tail("n", n, batch);
    if (rc == MATINV_OK) rc = check_count("ntarget", ntarget, "targets");
    if (rc == MATINV_OK && dGrad) rc = check_count("nparam", nparam, "derivative matrices");
    return rc;
}

// n <= 96: the gradient form of the trend tile kernels. Beyond, to n = 1024: that of the global-memory Cholesky kernel.
template <class T>
int trend_grad_dispatch(int n, int nbasis, int ntarget, int nparam, const void *dBs, const void *dCs, const void *dHs, const void *dYs,
                        const void *dDMs, void *dGrad, void *dGradC, void *dLogml, void *dAlpha, void *dBeta, size_t batch, int *dInfo,
                        hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *B = static_cast<const T *>(dBs), *c = static_cast<const T *>(dCs), *h = static_cast<const T *>(dHs);
    const T *y = static_cast<const T *>(dYs);
    const T *dM = dGrad ? static_cast<const T *>(dDMs) : nullptr;  // not read without grad
    T *grad = static_cast<T *>(dGrad), *gradc = static_cast<T *>(dGradC), *lm = static_cast<T *>(dLogml), *al = static_cast<T *>(dAlpha);
    T *be = static_cast<T *>(dBeta);
    const hipError_t e =
        trend_grad_tile_supports(n)
            ? launch_trend_grad_tile<T>(n, nbasis, ntarget, nparam, B, c, h, y, dM, grad, gradc, lm, al, be, batch, dInfo, stream)
            : launch_trend_grad_global<T>(n, nbasis, ntarget, nparam, B, c, h, y, dM, grad, gradc, lm, al, be, batch, dInfo, stream);
    if (e != hipSuccess) return fail_hip(e, "trend_grad launch");
    return MATINV_OK;
}

template <class T>
int trend_grad_host(int n, int nbasis, int ntarget, int nparam, const void *hBs, const void *hCs, const void *hHs, const void *hYs,
                    const void *hDMs, void *hGrad, void *hGradC, void *hLogml, void *hAlpha, void *hBeta, size_t batch, int *info)
{
    const size_t K = (size_t)nbasis, vec = (size_t)n * batch, mat = vec * n, ts = batch * (size_t)ntarget, ys = ts * n;
    const size_t par = hGrad ? batch * (size_t)nparam : 0;
    // the derivative matrices are read for grad only
    const StagedIn in[] = {{hBs, mat}, {hCs, vec}, {hHs, vec * K}, {hYs, ys}, {hGrad ? hDMs : nullptr, par * (size_t)n * n}};
    const StagedOut out[] = {{hGrad, par}, {hGradC, vec}, {hLogml, ts}, {hAlpha, ys}, {hBeta, ts * K}};
    return run_staged<T>("trend_grad", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return trend_grad_dispatch<T>(n, nbasis, ntarget, nparam, i[0], i[1], i[2], i[3], i[4], o[0], o[1], o[2], o[3], o[4], batch, dInfo,
                                      nullptr);
    });
}

// ---- leave-one-out cross-validation of the trend model (matinv_trend_loo_batched) --------------------------------------------------------
// the checks of trend_check_args, in its order; n <= nbasis leaves no held-out fit; var needs no targets
int trend_loo_check_args(int dtype, int n, int nbasis, int ntarget, const void *dBs, const void *dHs, const void *dYs, const void *dMean,
                         const void *dVar, const void *dLogPL, size_t batch)
{
    const bool targets = dMean || dLogPL;
    if (int rc = check_head("n", n, dtype)) return rc;
    if (nbasis < 1 || nbasis > 16) return fail(MATINV_ERR_ARG, "nbasis must be in 1 .. 16 (got %d)", nbasis);
    if (nbasis >= n) return fail(MATINV_ERR_ARG, "nbasis=%d leaves no held-out fit at n=%d: n - 1 points cannot carry the basis", nbasis, n);
    if (batch == 0) return MATINV_OK;
    if (targets && ntarget < 1) return fail(MATINV_ERR_ARG, "ntarget must be >= 1 with mean or logpl (got %d)", ntarget);
    if (!dBs || !dHs) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!targets && !dVar) return fail(MATINV_ERR_ARG, "no output requested (mean, var and logpl are all null)");
    if (targets && !dYs) return fail(MATINV_ERR_ARG, "mean or logpl requested without the targets (dYs is null)");
    int rc = check_tail("n", n, batch);
    if (rc == MATINV_OK && targets) rc = check_count("ntarget", ntarget, "targets");
    return rc;
}

// n <= 96: the leave-one-out form of the trend tile kernels. Beyond, to n = 1024: that of the global-memory Cholesky kernel.
template <class T>
int trend_loo_dispatch(int n, int nbasis, int ntarget, const void *dBs, const void *dCs, const void *dHs, const void *dYs, void *dMean,
                       void *dVar, void *dLogPL, size_t batch, int *dInfo, hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *B = static_cast<const T *>(dBs), *c = static_cast<const T *>(dCs), *h = static_cast<const T *>(dHs);
    T *mn = static_cast<T *>(dMean), *vr = static_cast<T *>(dVar), *lp = static_cast<T *>(dLogPL);
    const bool targets = mn || lp;
    const T *y = targets ? static_cast<const T *>(dYs) : nullptr;  // not read for var
    const int nd = targets ? ntarget : 0;
    const hipError_t e = trend_loo_tile_supports(n) ? launch_trend_loo_tile<T>(n, nbasis, nd, B, c, h, y, mn, vr, lp, batch, dInfo, stream)
                                                    : launch_trend_loo_global<T>(n, nbasis, nd, B, c, h, y, mn, vr, lp, batch, dInfo, stream);
    if (e != hipSuccess) return fail_hip(e, "trend_loo launch");
    return MATINV_OK;
}

template <class T>
int trend_loo_host(int n, int nbasis, int ntarget, const void *hBs, const void *hCs, const void *hHs, const void *hYs, void *hMean,
                   void *hVar, void *hLogPL, size_t batch, int *info)
{
    const bool targets = hMean || hLogPL;
    const size_t K = (size_t)nbasis, vec = (size_t)n * batch, mat = vec * n, ts = targets ? batch * (size_t)ntarget : 0;
    // the targets are read for mean and logpl only
    const StagedIn in[] = {{hBs, mat}, {hCs, vec}, {hHs, vec * K}, {targets ? hYs : nullptr, ts * n}};
    const StagedOut out[] = {{hMean, ts * n}, {hVar, vec}, {hLogPL, ts}};
    return run_staged<T>("trend_loo", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return trend_loo_dispatch<T>(n, nbasis, ntarget, i[0], i[1], i[2], i[3], o[0], o[1], o[2], batch, dInfo, nullptr);
    });
}

// ---- GP log marginal likelihood and its gradient from coordinates (matinv_ard_logml_batched) -------------------------------------------
// kind and ndim >= 1 are checked with n and dtype, as nbasis is in the trend families; ndim > 16 is a count limit
int ard_check_args(int dtype, int kind, int n, int ndim, const void *dXs, size_t xstride, const void *dYs, size_t ystride,
                   const void *dThetas, const void *dLogML, const void *dGrad, const void *dAlpha, size_t batch)
{
    if (int rc = check_head("n", n, dtype)) return rc;
    if (kind != MATINV_COV_SE && kind != MATINV_COV_MATERN52) return fail(MATINV_ERR_ARG, "unknown covariance function %d", kind);
    if (ndim < 1) return fail(MATINV_ERR_ARG, "ndim must be >= 1 (got %d)", ndim);
    if (batch == 0) return MATINV_OK;
    if (xstride != 0 && xstride != (size_t)n * (size_t)ndim)
        return fail(MATINV_ERR_ARG, "xstride must be n*ndim = %zu, or 0 for one shared point set (got %zu)", (size_t)n * (size_t)ndim, xstride);
    if (ystride != 0 && ystride != (size_t)n)
        return fail(MATINV_ERR_ARG, "ystride must be n = %d, or 0 for one shared target vector (got %zu)", n, ystride);
    if (!dXs || !dYs || !dThetas) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!dLogML && !dGrad && !dAlpha) return fail(MATINV_ERR_ARG, "no output requested (logml, grad and alpha are all null)");
    int rc = check_tail("n", n, batch);
    if (rc == MATINV_OK && ndim > ARD_MAX_DIM)
        rc = fail(MATINV_ERR_UNSUPPORTED, "ndim=%d exceeds the limit of %d dimensions per point", ndim, ARD_MAX_DIM);
    return rc;
}

// n <= 96: the ARD form of the SPD tile kernels. Beyond, to n = 1024: that of the global-memory Cholesky kernel.
template <class T>
int ard_dispatch(int kind, int n, int ndim, const void *dXs, size_t xstride, const void *dYs, size_t ystride, const void *dThetas,
                 void *dLogML, void *dGrad, void *dAlpha, size_t batch, int *dInfo, hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *x = static_cast<const T *>(dXs), *y = static_cast<const T *>(dYs), *th = static_cast<const T *>(dThetas);
    T *lm = static_cast<T *>(dLogML), *gr = static_cast<T *>(dGrad), *al = static_cast<T *>(dAlpha);
    const hipError_t e = ard_tile_supports(n) ? launch_ard_tile<T>(kind, n, ndim, x, xstride, y, ystride, th, lm, gr, al, batch, dInfo, stream)
                                              : launch_ard_global<T>(kind, n, ndim, x, xstride, y, ystride, th, lm, gr, al, batch, dInfo, stream);
    if (e != hipSuccess) return fail_hip(e, "ard_logml launch");
    return MATINV_OK;
}

template <class T>
int ard_host(int kind, int n, int ndim, const void *hXs, size_t xstride, const void *hYs, size_t ystride, const void *hThetas, void *hLogML,
             void *hGrad, void *hAlpha, size_t batch, int *info)
{
    const size_t pts = (size_t)n * ndim, P = (size_t)ndim + 2;
    // a shared point set or target vector (stride 0) is staged once, with its own count
    const StagedIn in[] = {{hXs, xstride ? batch * pts : pts}, {hYs, ystride ? batch * (size_t)n : (size_t)n}, {hThetas, batch * P}};
    const StagedOut out[] = {{hLogML, batch}, {hGrad, batch * P}, {hAlpha, batch * (size_t)n}};
    return run_staged<T>("ard_logml", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return ard_dispatch<T>(kind, n, ndim, i[0], xstride, i[1], ystride, i[2], o[0], o[1], o[2], batch, dInfo, nullptr);
    });
}

// ---- GP prediction from coordinates (matinv_ard_predict_batched) ------------------------------------------------------------------------
// the order of ard_check_args; nquery before the strides, the outputs as predict_check_args words them
int ard_predict_check_args(int dtype, int kind, int n, int ndim, int nquery, const void *dXs, size_t xstride, const void *dYs, size_t ystride,
                           const void *dThetas, const void *dXqs, size_t xqstride, const void *dMean, const void *dVar, size_t batch)
{
    if (int rc = check_head("n", n, dtype)) return rc;
    if (kind != MATINV_COV_SE && kind != MATINV_COV_MATERN52) return fail(MATINV_ERR_ARG, "unknown covariance function %d", kind);
    if (ndim < 1) return fail(MATINV_ERR_ARG, "ndim must be >= 1 (got %d)", ndim);
    if (batch == 0) return MATINV_OK;
    if (nquery < 1) return fail(MATINV_ERR_ARG, "nquery must be >= 1 (got %d)", nquery);
    if (xstride != 0 && xstride != (size_t)n * (size_t)ndim)
        return fail(MATINV_ERR_ARG, "xstride must be n*ndim = %zu, or 0 for one shared point set (got %zu)", (size_t)n * (size_t)ndim, xstride);
    if (ystride != 0 && ystride != (size_t)n)
        return fail(MATINV_ERR_ARG, "ystride must be n = %d, or 0 for one shared target vector (got %zu)", n, ystride);
    if (xqstride != 0 && xqstride != (size_t)nquery * (size_t)ndim)
        return fail(MATINV_ERR_ARG, "xqstride must be nquery*ndim = %zu, or 0 for one shared query set (got %zu)",
                    (size_t)nquery * (size_t)ndim, xqstride);
    if (!dXs || !dThetas || !dXqs) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!dMean && !dVar) return fail(MATINV_ERR_ARG, "no output requested (mean and var are both null)");
    if (dMean && !dYs) return fail(MATINV_ERR_ARG, "mean requested without the observations (dYs is null)");
    int rc = check_tail("n", n, batch);
    if (rc == MATINV_OK && ndim > ARD_MAX_DIM)
        rc = fail(MATINV_ERR_UNSUPPORTED, "ndim=%d exceeds the limit of %d dimensions per point", ndim, ARD_MAX_DIM);
    return rc;
}

// n <= 96: the ARD prediction form of the tile kernels. Beyond, to n = 1024: that of the global-memory kernel.
template <class T>
int ard_predict_dispatch(int kind, int n, int ndim, int nquery, const void *dXs, size_t xstride, const void *dYs, size_t ystride,
                         const void *dThetas, const void *dXqs, size_t xqstride, void *dMean, void *dVar, size_t batch, int *dInfo,
                         hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const T *x = static_cast<const T *>(dXs), *y = static_cast<const T *>(dYs), *th = static_cast<const T *>(dThetas);
    const T *xq = static_cast<const T *>(dXqs);
    T *mean = static_cast<T *>(dMean), *var = static_cast<T *>(dVar);
    const hipError_t e =
        ard_predict_tile_supports(n)
            ? launch_ard_predict_tile<T>(kind, n, ndim, nquery, x, xstride, y, ystride, th, xq, xqstride, mean, var, batch, dInfo, stream)
            : launch_ard_predict_global<T>(kind, n, ndim, nquery, x, xstride, y, ystride, th, xq, xqstride, mean, var, batch, dInfo, stream);
    if (e != hipSuccess) return fail_hip(e, "ard_predict launch");
    return MATINV_OK;
}

template <class T>
int ard_predict_host(int kind, int n, int ndim, int nquery, const void *hXs, size_t xstride, const void *hYs, size_t ystride,
                     const void *hThetas, const void *hXqs, size_t xqstride, void *hMean, void *hVar, size_t batch, int *info)
{
    const size_t pts = (size_t)n * ndim, qpts = (size_t)nquery * ndim, P = (size_t)ndim + 2, qs = batch * (size_t)nquery;
    // a shared point set, target vector or query set (stride 0) is staged once, with its own count; the targets are read for mean only
    const StagedIn in[] = {{hXs, xstride ? batch * pts : pts},
                           {hMean ? hYs : nullptr, ystride ? batch * (size_t)n : (size_t)n},
                           {hThetas, batch * P},
                           {hXqs, xqstride ? batch * qpts : qpts}};
    const StagedOut out[] = {{hMean, qs}, {hVar, qs}};
    return run_staged<T>("ard_predict", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return ard_predict_dispatch<T>(kind, n, ndim, nquery, i[0], xstride, i[1], ystride, i[2], i[3], xqstride, o[0], o[1], batch, dInfo,
                                       nullptr);
    });
}

// ---- batched joint posterior samples at the query points of a GP (matinv_sample_batched) -----------------------------------------------
int sample_check_args(int dtype, int n, int nquery, int nsample, const void *dBs, const void *dDs, const void *dAs, const void *dZs,
                      const void *dY, const void *dMean, size_t batch)
{
    if (int rc = check_head("n", n, dtype)) return rc;
    if (batch == 0) return MATINV_OK;
    if (nquery < 1) return fail(MATINV_ERR_ARG, "nquery must be >= 1 (got %d)", nquery);
    if (nsample < 1) return fail(MATINV_ERR_ARG, "nsample must be >= 1 (got %d)", nsample);
    if (!dBs || !dAs || !dZs) return fail(MATINV_ERR_ARG, "null device pointer");
    if (!dY) return fail(MATINV_ERR_ARG, "no output requested (Y is null)");
    if (dMean && !dDs) return fail(MATINV_ERR_ARG, "mean requested without the observations (dDs is null)");
    int rc = check_tail("n", n, batch);
    if (rc == MATINV_OK) rc = check_count("nquery", nquery, "query points");
    if (rc == MATINV_OK) rc = check_count("nsample", nsample, "samples");
    return rc;
}

// Two launches per k-range chunk: the predictive-covariance route for this n (unchanged), then the colour route for Q on its cov and mean.
// What the caller did not ask for goes into library scratch; the chunk is sized so that this scratch, together with the working copies the
// global forms of either route allocate for the same chunk, fits the blocked-path workspace cap. dDs == nullptr: the zero-mean posterior
// (no mean is computed, the colour route gets no m).
template <class T>
int sample_dispatch(int n, int nquery, int nsample, const void *dBs, const void *dCs, const void *dDs, const void *dAs, const void *dEs,
                    const void *dZs, void *dY, void *dMean, void *dCov, size_t batch, int *dInfo, hipStream_t stream)
{
    int rc = check_device();
    if (rc) return rc;
    const size_t Q = (size_t)nquery, qq = Q * Q, N = (size_t)n;
    const T *B = static_cast<const T *>(dBs), *c = static_cast<const T *>(dCs), *d = static_cast<const T *>(dDs);
    const T *a = static_cast<const T *>(dAs), *e_ = static_cast<const T *>(dEs), *z = static_cast<const T *>(dZs);
    T *Y = static_cast<T *>(dY), *mean = static_cast<T *>(dMean), *cov = static_cast<T *>(dCov);
    const bool own_mean = d && !mean, own_cov = !cov;
    const size_t own = (own_mean ? Q : 0) + (own_cov ? qq : 0);
    size_t chunk = batch;
    T *ws = nullptr;
    hipError_t e = hipSuccess;
    if (own) {
        const size_t per = own + (predict_cov_tile_supports(n) ? 0 : N * (N + Q)) + (colour_tile_supports(nquery) ? 0 : qq);
        chunk = blocked_workspace_cap() / (per * sizeof(T));
        if (chunk < 1) chunk = 1;
        if (chunk > batch) chunk = batch;
        e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * own * sizeof(T), stream);
        if (e != hipSuccess) return fail_hip(e, "sample workspace");
    }
    for (size_t off = 0; off < batch && rc == MATINV_OK; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        T *const cmean = !d ? nullptr : own_mean ? ws : mean + off * Q;
        T *const ccov = own_cov ? ws + (own_mean ? chunk * Q : 0) : cov + off * qq;
        int *const cinfo = dInfo ? dInfo + off : nullptr;
        rc = predict_cov_dispatch<T>(n, nquery, B + off * N * N, c ? c + off * N : nullptr, d ? d + off * N : nullptr, a + off * Q * N,
                                     e_ ? e_ + off * qq : nullptr, cmean, ccov, cnt, cinfo, stream);
        if (rc == MATINV_OK)
            rc = colour_dispatch<T>(nquery, nsample, ccov, qq, cmean, z + off * Q * nsample, Y + off * Q * nsample, nullptr, cnt, cinfo, n,
                                    stream);
    }
    if (ws) {
        const hipError_t e2 = scratch_free(ws, stream);
        if (rc == MATINV_OK && e2 != hipSuccess) return fail_hip(e2, "sample workspace");
    }
    return rc;
}

template <class T>
int sample_host(int n, int nquery, int nsample, const void *hBs, const void *hCs, const void *hDs, const void *hAs, const void *hEs,
                const void *hZs, void *hY, void *hMean, void *hCov, size_t batch, int *info)
{
    const size_t vec = (size_t)n * batch, mat = vec * n, qs = batch * (size_t)nquery, qq = qs * (size_t)nquery, ys = qs * (size_t)nsample;
    // the observations and the prior covariances go along whenever they are given: without Ds the posterior has zero mean
    const StagedIn in[] = {{hBs, mat}, {hCs, vec}, {hDs, vec}, {hAs, qs * (size_t)n}, {hEs, qq}, {hZs, ys}};
    const StagedOut out[] = {{hY, ys}, {hMean, qs}, {hCov, qq}};
    return run_staged<T>("sample", in, out, batch, info, [&](T *const *i, T *const *o, int *dInfo) {
        return sample_dispatch<T>(n, nquery, nsample, i[0], i[1], i[2], i[3], i[4], i[5], o[0], o[1], o[2], batch, dInfo, nullptr);
    });
}

template <class T>
int lu_kernel(int n)
{
    return (n > 16 && (tilep_supports(n) || tileq_supports(sizeof(T) == 8, n))) ? (int)MATINV_KERNEL_TILEP : (int)MATINV_KERNEL_AUTO;
}

// Reference error contract: message on stderr, then exit (include/helper_gpu.h:9-18, helper_cpu.h:12-21 there).
void die_on(int rc, const char *fn)
{
    if (rc == MATINV_OK) return;
    fprintf(stderr, "ENSURE FAILED %s\r\n%s\r\n", fn, g_err);
    if (errno) perror("possible reason for failure from ERRNO");
    (void)hipDeviceReset();
    exit(EXIT_FAILURE);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
extern "C" {

int matinv_abi_version(void) { return 2; }  // 2 (r03): + matinv_queue_*, matinv_batched_*, matinv_set_gj_policy, *_host_multi, matinv_allgather_*

int matinv_set_gj_policy(int policy)
{
    if (policy != MATINV_GJ_NATURAL_FIRST && policy != MATINV_GJ_PIVOT && policy != MATINV_GJ_ADAPTIVE)
        return fail(MATINV_ERR_ARG, "unknown Gauss-Jordan policy %d", policy);
    return set_gj_policy(policy);
}

int matinv_shard_range(size_t batch, int nshards, int n, int g, size_t *lo, size_t *hi)
{
    if (nshards < 1 || g < 0 || g >= nshards || n < 1 || !lo || !hi) return fail(MATINV_ERR_ARG, "matinv_shard_range: bad argument");
    shard_range(batch, nshards, n, g, *lo, *hi);
    return MATINV_OK;
}

int matinv_device_count(void)
{
    std::vector<int> devs;
    int rc = gfx950_devices(devs);
    return rc ? rc : (int)devs.size();
}

int matinv_inverse_batched_host_multi(int algo, int dtype, int n, const void *hA, void *hAinv, size_t batch, int *info, int nshards)
{
    return by_dtype(dtype, [&](auto t) {
        return inverse_host_multi<decltype(t)>(algo, n, hA, hAinv, batch, info, nshards, MATINV_KERNEL_AUTO);
    });
}

int matinv_release_cache(void)
{
    int rc = check_device();
    if (rc) return rc;
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail_hip(e, "release cache");
    blocked_gp_release_graphs();
    scratch_release_device();
    return MATINV_OK;
}
int matinv_stream_retire(void *stream)
{
    if (!stream) return fail(MATINV_ERR_ARG, "matinv_stream_retire: the null stream is never retired");
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, "stream retire");
    scratch_retire_stream(static_cast<hipStream_t>(stream));
    return MATINV_OK;
}
long long matinv_debug_rejects(int reset) { return debug_rejects(reset != 0); }
const char *matinv_last_error(void) { return g_err; }

// batchedCudaMalloc (/root/reference/src/helper.cu:103-118): ONE pitched device block, host table of row pointers.
int matinv_batched_malloc(void **devArrayPtr, size_t *pitch, size_t arraySize, int batchSize)
{
    if (!devArrayPtr || !pitch || batchSize < 0) return fail(MATINV_ERR_ARG, "matinv_batched_malloc: bad argument");
    if (batchSize == 0 || arraySize == 0) {
        *pitch = arraySize;
        return MATINV_OK;
    }
    int rc = check_device();
    if (rc) return rc;
    char *p = nullptr;
    hipError_t e = hipMallocPitch(reinterpret_cast<void **>(&p), pitch, arraySize, (size_t)batchSize);
    if (e != hipSuccess) return fail_hip(e, "hipMallocPitch");
    for (int i = 0; i < batchSize; ++i) devArrayPtr[i] = p + (size_t)i * *pitch;
    return MATINV_OK;
}

int matinv_batched_free(void **devArrayPtr)
{
    if (!devArrayPtr || !devArrayPtr[0]) return MATINV_OK;
    hipError_t e = hipFree(devArrayPtr[0]);
    if (e != hipSuccess) return fail_hip(e, "hipFree");
    devArrayPtr[0] = nullptr;
    return MATINV_OK;
}

// cudaMemcpy2D as the reference uses it on those blocks (src/gauss_bench.cu:165-170,244): blocking, default stream
int matinv_memcpy_2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, int toDevice)
{
    if (width == 0 || height == 0) return MATINV_OK;
    if (!dst || !src || dpitch < width || spitch < width) return fail(MATINV_ERR_ARG, "matinv_memcpy_2d: bad argument");
    hipError_t e = hipMemcpy2D(dst, dpitch, src, spitch, width, height, toDevice ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail_hip(e, "hipMemcpy2D");
    return MATINV_OK;
}

// how the adaptive Gauss-Jordan dispatch of the tile family went (tile_kernels.hip "natural order or pivot search?")
int matinv_tile_stats(unsigned long long *natural_launches, unsigned long long *pivot_launches, unsigned long long *last_rejected,
                      unsigned long long *last_batch)
{
    const TileStats s = tile_stats();
    if (natural_launches) *natural_launches = s.natural_launches;
    if (pivot_launches) *pivot_launches = s.pivot_launches;
    if (last_rejected) *last_rejected = s.last_rejected;
    if (last_batch) *last_batch = s.last_batch;
    return MATINV_OK;
}

// which route the unscreened 64 x 64 fp64 Gauss-Jordan launches took (tile_kernels.hip "symmetric-only kernel in front")
int matinv_sym_front_stats(unsigned long long *front_launches, unsigned long long *direct_launches, unsigned long long *last_not_symmetric,
                           unsigned long long *last_batch)
{
    const SymFrontStats s = sym_front_stats();
    if (front_launches) *front_launches = s.front_launches;
    if (direct_launches) *direct_launches = s.direct_launches;
    if (last_not_symmetric) *last_not_symmetric = s.last_not_symmetric;
    if (last_batch) *last_batch = s.last_batch;
    return MATINV_OK;
}

int matinv_device_synchronize(void)
{
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail_hip(e, "hipDeviceSynchronize");
    return MATINV_OK;
}

int matinv_inverse_batched_ex(int algo, int dtype, int n, const void *dA, size_t strideA, void *dAinv,
                              size_t strideInv, size_t batch, int *dInfo, void *stream, int kernel)
{
    return by_dtype(dtype, [&](auto t) {
        return inverse_strided<decltype(t)>(algo, n, dA, strideA, dAinv, strideInv, batch, dInfo, stream, kernel);
    });
}

int matinv_inverse_batched(int algo, int dtype, int n, const void *dA, size_t strideA, void *dAinv, size_t strideInv,
                           size_t batch, int *dInfo, void *stream)
{
    return matinv_inverse_batched_ex(algo, dtype, n, dA, strideA, dAinv, strideInv, batch, dInfo, stream,
                                     MATINV_KERNEL_AUTO);
}

int matinv_select_kernel(int algo, int dtype, int n)
{
    if (int rc = check_order("n", n)) return rc;
    int k = (dtype == MATINV_F64) ? select_auto<double>(algo, n) : select_auto<float>(algo, n);
    if (k < 0) return fail(MATINV_ERR_UNSUPPORTED, "n=%d exceeds every kernel family built in", n);
    return k;
}

const char *matinv_kernel_name(int algo, int dtype, int n, int kernel)
{
    const bool f64 = dtype == MATINV_F64;
    if (n < 1 || (dtype != MATINV_F64 && dtype != MATINV_F32) || (algo != MATINV_ALGO_GAUSS_JORDAN && algo != MATINV_ALGO_CHOLESKY)) return "";
    if (kernel == MATINV_KERNEL_AUTO) kernel = f64 ? select_auto<double>(algo, n) : select_auto<float>(algo, n);
    // "" exactly where inverse_dispatch answers MATINV_ERR_UNSUPPORTED (a forced family that has no kernel for this n)
    if (!(f64 ? family_serves<double>(algo, n, kernel) : family_serves<float>(algo, n, kernel))) return "";
    switch (kernel) {
    case MATINV_KERNEL_LDS: return algo == MATINV_ALGO_CHOLESKY ? name_chol_lds(f64) : name_gj_lds(f64);
    case MATINV_KERNEL_ROWLANE: return algo == MATINV_ALGO_CHOLESKY ? name_spd_rowlane(f64, n) : name_gj_rowlane(f64, n);
    case MATINV_KERNEL_TILE: return algo == MATINV_ALGO_CHOLESKY ? name_spd_tile(f64, n) : name_gj_tile(f64, n);
    case MATINV_KERNEL_ROW: return name_gj_row(f64, n);
    case MATINV_KERNEL_TILEP: return n > 128 ? name_gj_tileq(f64, n) : name_gj_tilep(f64, n);
    case MATINV_KERNEL_GLOBAL: return algo == MATINV_ALGO_CHOLESKY ? name_chol_global(f64) : name_gj_global(f64);
    case MATINV_KERNEL_BLOCKED:
        if (algo == MATINV_ALGO_GAUSS_JORDAN) {
            // the kernel that dominates: the rank-128 MFMA update of the two-level scheme, the rank-32 VALU update below its threshold
            if (n < blocked_gj_two_level_min()) return f64 ? "matinv_bgj_update1<double>" : "matinv_bgj_update1<float>";
            return f64 ? "matinv_bgj_update_mfma<double, false, 2, 2>" : "matinv_bgj_update_mfma<float, false, 2, 2>";
        }
        return f64 ? "matinv_bgp_update<double>" : "matinv_bgp_update<float>";  // the trailing update: most of the time
    default: return "";
    }
}

int matinv_solve_batched_ex(int algo, int dtype, int n, int nrhs, const void *dA, size_t strideA, const void *dB, size_t strideB, void *dX,
                            size_t strideX, size_t batch, int *dInfo, void *stream, int kernel)
{
    int rc = solve_check_args(algo, dtype, n, nrhs, dA, strideA, dB, strideB, dX, strideX, batch, kernel);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return solve_strided<decltype(t)>(algo, n, nrhs, dA, strideA, dB, strideB, dX, strideX, batch, dInfo, st, kernel);
    });
}

int matinv_solve_batched(int algo, int dtype, int n, int nrhs, const void *dA, size_t strideA, const void *dB, size_t strideB, void *dX,
                         size_t strideX, size_t batch, int *dInfo, void *stream)
{
    return matinv_solve_batched_ex(algo, dtype, n, nrhs, dA, strideA, dB, strideB, dX, strideX, batch, dInfo, stream, MATINV_KERNEL_AUTO);
}

const char *matinv_solve_kernel_name(int algo, int dtype, int n, int nrhs, int kernel)
{
    if (solve_check_args(algo, dtype, n, nrhs, nullptr, 0, nullptr, 0, nullptr, 0, 0, kernel) != MATINV_OK || n > 1024) return "";
    int family = MATINV_KERNEL_AUTO;
    const int route = solve_route(algo, n, nrhs, kernel, family);
    const bool f64 = dtype == MATINV_F64;
    if (route == SOLVE_FUSED) return name_solve_tile(f64, algo == MATINV_ALGO_CHOLESKY, n);
    if (route == SOLVE_ROW) return name_solve_row(f64, n, nrhs);
    if (route == SOLVE_COMPOSED) return matinv_kernel_name(algo, dtype, n, family);
    return "";
}

int matinv_solve_batched_host(int algo, int dtype, int n, int nrhs, const void *hA, const void *hB, void *hX, size_t batch, int *info)
{
    int rc = solve_check_args(algo, dtype, n, nrhs, hA, (size_t)n * n, hB, (size_t)n * nrhs, hX, (size_t)n * nrhs, batch,
                              MATINV_KERNEL_AUTO);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) { return solve_host<decltype(t)>(algo, n, nrhs, hA, hB, hX, batch, info); });
}

int matinv_logdet_batched_ex(int algo, int dtype, int n, const void *dA, size_t strideA, void *dLogAbsDet, void *dSign, size_t batch,
                             int *dInfo, void *stream, int kernel)
{
    int rc = logdet_check_args(algo, dtype, n, dA, strideA, dLogAbsDet, batch, kernel);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return logdet_strided<decltype(t)>(algo, n, dA, strideA, dLogAbsDet, dSign, batch, dInfo, st, kernel);
    });
}

int matinv_logdet_batched(int algo, int dtype, int n, const void *dA, size_t strideA, void *dLogAbsDet, void *dSign, size_t batch,
                          int *dInfo, void *stream)
{
    return matinv_logdet_batched_ex(algo, dtype, n, dA, strideA, dLogAbsDet, dSign, batch, dInfo, stream, MATINV_KERNEL_AUTO);
}

const char *matinv_logdet_kernel_name(int algo, int dtype, int n, int kernel)
{
    if (logdet_check_args(algo, dtype, n, nullptr, 0, nullptr, 0, kernel) != MATINV_OK || n > 1024) return "";
    const int route = logdet_route(algo, n, kernel);
    const bool f64 = dtype == MATINV_F64;
    if (route == LOGDET_TILE) return name_logdet_tile(f64, false, n);
    if (route == LOGDET_ROW) return name_logdet_row(f64, n);
    if (route == LOGDET_GLOBAL) return name_logdet_global(f64, algo == MATINV_ALGO_CHOLESKY);
    return "";
}

const char *matinv_gp_kernel_name(int dtype, int n, int variance)
{
    (void)variance;  // mean and variance are one instantiation: the form is chosen by a null pointer at run time
    if (n < 1 || (dtype != MATINV_F64 && dtype != MATINV_F32)) return "";
    const bool f64 = dtype == MATINV_F64;
    switch (f64 ? gp_route<double>(n) : gp_route<float>(n)) {
    case GP_ROWLANE: return name_gp_rowlane(f64, n);
    case GP_ROWLANE2: return name_gp_rowlane2(f64, n);
    case GP_SPD_TILE2: return name_spd_tile2(true, n);
    case GP_SPD_TILE: return name_gp_spd_tile(f64, n);
    case GP_TILE: return name_gp_tile(f64, n);
    case GP_BLOCKED: return f64 ? "matinv_bgp_update<double>" : "matinv_bgp_update<float>";  // the trailing update: most of the time
    default: return "";
    }
}

const char *matinv_logml_kernel_name(int dtype, int n)
{
    if (logml_check_args(dtype, n, nullptr, nullptr, nullptr, 0) != MATINV_OK || n > 1024) return "";
    // composed: the variance pipeline does the work that grows fastest (then matinv_logdet_global and matinv_logml_combine)
    return logml_route(n) == LOGML_TILE ? name_logdet_tile(dtype == MATINV_F64, true, n) : matinv_gp_kernel_name(dtype, n, 1);
}

int matinv_logdet_batched_host(int algo, int dtype, int n, const void *hA, void *hLogAbsDet, void *hSign, size_t batch, int *info)
{
    int rc = logdet_check_args(algo, dtype, n, hA, (size_t)n * n, hLogAbsDet, batch, MATINV_KERNEL_AUTO);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) { return logdet_host<decltype(t)>(algo, n, hA, hLogAbsDet, hSign, batch, info); });
}

int matinv_logml_batched(int dtype, int n, const void *dBs, const void *dCs, const void *dDs, void *dLogml, size_t batch, int *dInfo,
                         void *stream)
{
    int rc = logml_check_args(dtype, n, dBs, dDs, dLogml, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) { return logml_dispatch<decltype(t)>(n, dBs, dCs, dDs, dLogml, batch, dInfo, st); });
}

int matinv_logml_batched_host(int dtype, int n, const void *hBs, const void *hCs, const void *hDs, void *hLogml, size_t batch, int *info)
{
    int rc = logml_check_args(dtype, n, hBs, hDs, hLogml, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) { return logml_host<decltype(t)>(n, hBs, hCs, hDs, hLogml, batch, info); });
}

int matinv_loo_batched(int dtype, int n, const void *dBs, const void *dCs, const void *dDs, void *dMean, void *dVar, void *dLogPL, size_t batch,
                       int *dInfo, void *stream)
{
    int rc = loo_check_args(dtype, n, dBs, dDs, dMean, dVar, dLogPL, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) { return loo_dispatch<decltype(t)>(n, dBs, dCs, dDs, dMean, dVar, dLogPL, batch, dInfo, st); });
}

const char *matinv_loo_kernel_name(int dtype, int n)
{
    if (!has_kernel_name(dtype, n)) return "";
    return loo_tile_supports(n) ? name_loo_tile(dtype == MATINV_F64, n) : name_loo_global(dtype == MATINV_F64);
}

int matinv_loo_batched_host(int dtype, int n, const void *hBs, const void *hCs, const void *hDs, void *hMean, void *hVar, void *hLogPL,
                            size_t batch, int *info)
{
    int rc = loo_check_args(dtype, n, hBs, hDs, hMean, hVar, hLogPL, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) { return loo_host<decltype(t)>(n, hBs, hCs, hDs, hMean, hVar, hLogPL, batch, info); });
}

int matinv_logml_grad_batched(int dtype, int n, int nparam, const void *dBs, const void *dCs, const void *dDs, const void *dDMs, void *dGrad,
                              void *dGradC, void *dAlpha, size_t batch, int *dInfo, void *stream)
{
    int rc = logml_grad_check_args(dtype, n, nparam, dBs, dDs, dDMs, dGrad, dGradC, dAlpha, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return logml_grad_dispatch<decltype(t)>(n, nparam, dBs, dCs, dDs, dDMs, dGrad, dGradC, dAlpha, batch, dInfo, st);
    });
}

const char *matinv_logml_grad_kernel_name(int dtype, int n)
{
    if (!has_kernel_name(dtype, n)) return "";
    return logml_grad_tile_supports(n) ? name_logml_grad_tile(dtype == MATINV_F64, n) : name_logml_grad_global(dtype == MATINV_F64);
}

int matinv_logml_grad_batched_host(int dtype, int n, int nparam, const void *hBs, const void *hCs, const void *hDs, const void *hDMs,
                                   void *hGrad, void *hGradC, void *hAlpha, size_t batch, int *info)
{
    int rc = logml_grad_check_args(dtype, n, nparam, hBs, hDs, hDMs, hGrad, hGradC, hAlpha, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) {
        return logml_grad_host<decltype(t)>(n, nparam, hBs, hCs, hDs, hDMs, hGrad, hGradC, hAlpha, batch, info);
    });
}

int matinv_predict_batched(int dtype, int n, int nquery, const void *dBs, const void *dCs, const void *dDs, const void *dAs, const void *dEs,
                           void *dMean, void *dVar, size_t batch, int *dInfo, void *stream)
{
    int rc = predict_check_args(dtype, n, nquery, dBs, dDs, dAs, dMean, dVar, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return predict_dispatch<decltype(t)>(n, nquery, dBs, dCs, dDs, dAs, dEs, dMean, dVar, batch, dInfo, st);
    });
}

const char *matinv_predict_kernel_name(int dtype, int n)
{
    if (!has_kernel_name(dtype, n)) return "";
    return predict_tile_supports(n) ? name_predict_tile(dtype == MATINV_F64, n) : name_predict_global(dtype == MATINV_F64);
}

int matinv_predict_batched_host(int dtype, int n, int nquery, const void *hBs, const void *hCs, const void *hDs, const void *hAs,
                                const void *hEs, void *hMean, void *hVar, size_t batch, int *info)
{
    int rc = predict_check_args(dtype, n, nquery, hBs, hDs, hAs, hMean, hVar, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) { return predict_host<decltype(t)>(n, nquery, hBs, hCs, hDs, hAs, hEs, hMean, hVar, batch, info); });
}

int matinv_predict_cov_batched(int dtype, int n, int nquery, const void *dBs, const void *dCs, const void *dDs, const void *dAs,
                               const void *dEs, void *dMean, void *dCov, size_t batch, int *dInfo, void *stream)
{
    int rc = predict_cov_check_args(dtype, n, nquery, dBs, dDs, dAs, dMean, dCov, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return predict_cov_dispatch<decltype(t)>(n, nquery, dBs, dCs, dDs, dAs, dEs, dMean, dCov, batch, dInfo, st);
    });
}

const char *matinv_predict_cov_kernel_name(int dtype, int n)
{
    if (!has_kernel_name(dtype, n)) return "";
    return predict_cov_tile_supports(n) ? name_predict_cov_tile(dtype == MATINV_F64, n) : name_predict_cov_global(dtype == MATINV_F64);
}

int matinv_predict_cov_batched_host(int dtype, int n, int nquery, const void *hBs, const void *hCs, const void *hDs, const void *hAs,
                                    const void *hEs, void *hMean, void *hCov, size_t batch, int *info)
{
    int rc = predict_cov_check_args(dtype, n, nquery, hBs, hDs, hAs, hMean, hCov, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) {
        return predict_cov_host<decltype(t)>(n, nquery, hBs, hCs, hDs, hAs, hEs, hMean, hCov, batch, info);
    });
}

int matinv_colour_batched(int dtype, int q, int nsample, const void *dC, size_t strideC, const void *dM, const void *dZ, void *dY, void *dL,
                          size_t batch, int *dInfo, void *stream)
{
    int rc = colour_check_args(dtype, q, nsample, dC, strideC, dZ, dY, dL, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return colour_dispatch<decltype(t)>(q, nsample, dC, strideC, dM, dZ, dY, dL, batch, dInfo, 0, st);
    });
}

const char *matinv_colour_kernel_name(int dtype, int q)
{
    if (!has_kernel_name(dtype, q)) return "";
    return colour_tile_supports(q) ? name_colour_tile(dtype == MATINV_F64, q) : name_colour_global(dtype == MATINV_F64);
}

int matinv_colour_batched_host(int dtype, int q, int nsample, const void *hC, size_t strideC, const void *hM, const void *hZ, void *hY,
                               void *hL, size_t batch, int *info)
{
    int rc = colour_check_args(dtype, q, nsample, hC, strideC, hZ, hY, hL, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) { return colour_host<decltype(t)>(q, nsample, hC, strideC, hM, hZ, hY, hL, batch, info); });
}

int matinv_whiten_batched(int dtype, int q, int npoint, const void *dC, size_t strideC, const void *dM, const void *dX, void *dW, void *dMaha,
                          void *dLogdet, void *dLogpdf, size_t batch, int *dInfo, void *stream)
{
    int rc = whiten_check_args(dtype, q, npoint, dC, strideC, dX, dW, dMaha, dLogdet, dLogpdf, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return whiten_dispatch<decltype(t)>(q, npoint, dC, strideC, dM, dX, dW, dMaha, dLogdet, dLogpdf, batch, dInfo, st);
    });
}

const char *matinv_whiten_kernel_name(int dtype, int q)
{
    if (!has_kernel_name(dtype, q)) return "";
    return whiten_tile_supports(q) ? name_whiten_tile(dtype == MATINV_F64, q) : name_whiten_global(dtype == MATINV_F64);
}

int matinv_whiten_batched_host(int dtype, int q, int npoint, const void *hC, size_t strideC, const void *hM, const void *hX, void *hW,
                               void *hMaha, void *hLogdet, void *hLogpdf, size_t batch, int *info)
{
    int rc = whiten_check_args(dtype, q, npoint, hC, strideC, hX, hW, hMaha, hLogdet, hLogpdf, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) {
        return whiten_host<decltype(t)>(q, npoint, hC, strideC, hM, hX, hW, hMaha, hLogdet, hLogpdf, batch, info);
    });
}

int matinv_multi_target_batched(int dtype, int n, int ntarget, int nquery, const void *dBs, const void *dCs, const void *dYs, const void *dAs,
                                void *dAlpha, void *dQuad, void *dLogdet, void *dLogml, void *dMean, size_t batch, int *dInfo, void *stream)
{
    int rc = multi_target_check_args(dtype, n, ntarget, nquery, dBs, dYs, dAs, dAlpha, dQuad, dLogdet, dLogml, dMean, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return multi_target_dispatch<decltype(t)>(n, ntarget, nquery, dBs, dCs, dYs, dAs, dAlpha, dQuad, dLogdet, dLogml, dMean, batch, dInfo,
                                                  st);
    });
}

const char *matinv_multi_target_kernel_name(int dtype, int n)
{
    if (!has_kernel_name(dtype, n)) return "";
    return multi_target_tile_supports(n) ? name_multi_target_tile(dtype == MATINV_F64, n) : name_multi_target_global(dtype == MATINV_F64);
}

int matinv_multi_target_batched_host(int dtype, int n, int ntarget, int nquery, const void *hBs, const void *hCs, const void *hYs,
                                     const void *hAs, void *hAlpha, void *hQuad, void *hLogdet, void *hLogml, void *hMean, size_t batch,
                                     int *info)
{
    int rc = multi_target_check_args(dtype, n, ntarget, nquery, hBs, hYs, hAs, hAlpha, hQuad, hLogdet, hLogml, hMean, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) {
        return multi_target_host<decltype(t)>(n, ntarget, nquery, hBs, hCs, hYs, hAs, hAlpha, hQuad, hLogdet, hLogml, hMean, batch, info);
    });
}

int matinv_multi_target_grad_batched(int dtype, int n, int ntarget, int nparam, const void *dBs, const void *dCs, const void *dYs,
                                     const void *dDMs, void *dGrad, void *dGradC, void *dLogml, void *dAlpha, size_t batch, int *dInfo,
                                     void *stream)
{
    int rc = multi_target_grad_check_args(dtype, n, ntarget, nparam, dBs, dYs, dDMs, dGrad, dGradC, dLogml, dAlpha, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return multi_target_grad_dispatch<decltype(t)>(n, ntarget, nparam, dBs, dCs, dYs, dDMs, dGrad, dGradC, dLogml, dAlpha, batch, dInfo, st);
    });
}

const char *matinv_multi_target_grad_kernel_name(int dtype, int n)
{
    if (!has_kernel_name(dtype, n)) return "";
    return multi_target_grad_tile_supports(n) ? name_multi_target_grad_tile(dtype == MATINV_F64, n)
                                              : name_multi_target_grad_global(dtype == MATINV_F64);
}

int matinv_multi_target_grad_batched_host(int dtype, int n, int ntarget, int nparam, const void *hBs, const void *hCs, const void *hYs,
                                          const void *hDMs, void *hGrad, void *hGradC, void *hLogml, void *hAlpha, size_t batch, int *info)
{
    int rc = multi_target_grad_check_args(dtype, n, ntarget, nparam, hBs, hYs, hDMs, hGrad, hGradC, hLogml, hAlpha, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) {
        return multi_target_grad_host<decltype(t)>(n, ntarget, nparam, hBs, hCs, hYs, hDMs, hGrad, hGradC, hLogml, hAlpha, batch, info);
    });
}

int matinv_trend_batched(int dtype, int n, int nbasis, int ntarget, int nquery, const void *dBs, const void *dCs, const void *dHs,
                         const void *dYs, const void *dAs, const void *dGs, const void *dEs, void *dBeta, void *dCovBeta, void *dAlpha,
                         void *dQuad, void *dLogml, void *dMean, void *dVar, size_t batch, int *dInfo, void *stream)
{
    int rc = trend_check_args(dtype, n, nbasis, ntarget, nquery, dBs, dHs, dYs, dAs, dGs, dEs, dBeta, dCovBeta, dAlpha, dQuad, dLogml, dMean,
                              dVar, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return trend_dispatch<decltype(t)>(n, nbasis, ntarget, nquery, dBs, dCs, dHs, dYs, dAs, dGs, dEs, dBeta, dCovBeta, dAlpha, dQuad, dLogml,
                                           dMean, dVar, batch, dInfo, st);
    });
}

const char *matinv_trend_kernel_name(int dtype, int n)
{
    if (!has_kernel_name(dtype, n)) return "";
    return trend_tile_supports(n) ? name_trend_tile(dtype == MATINV_F64, n) : name_trend_global(dtype == MATINV_F64);
}

int matinv_trend_batched_host(int dtype, int n, int nbasis, int ntarget, int nquery, const void *hBs, const void *hCs, const void *hHs,
                              const void *hYs, const void *hAs, const void *hGs, const void *hEs, void *hBeta, void *hCovBeta, void *hAlpha,
                              void *hQuad, void *hLogml, void *hMean, void *hVar, size_t batch, int *info)
{
    int rc = trend_check_args(dtype, n, nbasis, ntarget, nquery, hBs, hHs, hYs, hAs, hGs, hEs, hBeta, hCovBeta, hAlpha, hQuad, hLogml, hMean,
                              hVar, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) {
        return trend_host<decltype(t)>(n, nbasis, ntarget, nquery, hBs, hCs, hHs, hYs, hAs, hGs, hEs, hBeta, hCovBeta, hAlpha, hQuad, hLogml,
                                       hMean, hVar, batch, info);
    });
}

int matinv_trend_grad_batched(int dtype, int n, int nbasis, int ntarget, int nparam, const void *dBs, const void *dCs, const void *dHs,
                              const void *dYs, const void *dDMs, void *dGrad, void *dGradC, void *dLogml, void *dAlpha, void *dBeta,
                              size_t batch, int *dInfo, void *stream)
{
    int rc = trend_grad_check_args(dtype, n, nbasis, ntarget, nparam, dBs, dHs, dYs, dDMs, dGrad, dGradC, dLogml, dAlpha, dBeta, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return trend_grad_dispatch<decltype(t)>(n, nbasis, ntarget, nparam, dBs, dCs, dHs, dYs, dDMs, dGrad, dGradC, dLogml, dAlpha, dBeta,
                                                batch, dInfo, st);
    });
}

const char *matinv_trend_grad_kernel_name(int dtype, int n)
{
    if (!has_kernel_name(dtype, n)) return "";
    return trend_grad_tile_supports(n) ? name_trend_grad_tile(dtype == MATINV_F64, n) : name_trend_grad_global(dtype == MATINV_F64);
}

int matinv_trend_grad_batched_host(int dtype, int n, int nbasis, int ntarget, int nparam, const void *hBs, const void *hCs, const void *hHs,
                                   const void *hYs, const void *hDMs, void *hGrad, void *hGradC, void *hLogml, void *hAlpha, void *hBeta,
                                   size_t batch, int *info)
{
    int rc = trend_grad_check_args(dtype, n, nbasis, ntarget, nparam, hBs, hHs, hYs, hDMs, hGrad, hGradC, hLogml, hAlpha, hBeta, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) {
        return trend_grad_host<decltype(t)>(n, nbasis, ntarget, nparam, hBs, hCs, hHs, hYs, hDMs, hGrad, hGradC, hLogml, hAlpha, hBeta, batch,
                                            info);
    });
}

int matinv_trend_loo_batched(int dtype, int n, int nbasis, int ntarget, const void *dBs, const void *dCs, const void *dHs, const void *dYs,
                             void *dMean, void *dVar, void *dLogPL, size_t batch, int *dInfo, void *stream)
{
    int rc = trend_loo_check_args(dtype, n, nbasis, ntarget, dBs, dHs, dYs, dMean, dVar, dLogPL, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return trend_loo_dispatch<decltype(t)>(n, nbasis, ntarget, dBs, dCs, dHs, dYs, dMean, dVar, dLogPL, batch, dInfo, st);
    });
}

// "" below n = 2 as well: with nbasis >= 1 no held-out fit exists at n = 1
const char *matinv_trend_loo_kernel_name(int dtype, int n)
{
    if (!has_kernel_name(dtype, n) || n < 2) return "";
    return trend_loo_tile_supports(n) ? name_trend_loo_tile(dtype == MATINV_F64, n) : name_trend_loo_global(dtype == MATINV_F64);
}

int matinv_trend_loo_batched_host(int dtype, int n, int nbasis, int ntarget, const void *hBs, const void *hCs, const void *hHs,
                                  const void *hYs, void *hMean, void *hVar, void *hLogPL, size_t batch, int *info)
{
    int rc = trend_loo_check_args(dtype, n, nbasis, ntarget, hBs, hHs, hYs, hMean, hVar, hLogPL, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) {
        return trend_loo_host<decltype(t)>(n, nbasis, ntarget, hBs, hCs, hHs, hYs, hMean, hVar, hLogPL, batch, info);
    });
}

int matinv_ard_logml_batched(int dtype, int kind, int n, int ndim, const void *dXs, size_t xstride, const void *dYs, size_t ystride,
                             const void *dThetas, void *dLogML, void *dGrad, void *dAlpha, size_t batch, int *dInfo, void *stream)
{
    int rc = ard_check_args(dtype, kind, n, ndim, dXs, xstride, dYs, ystride, dThetas, dLogML, dGrad, dAlpha, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return ard_dispatch<decltype(t)>(kind, n, ndim, dXs, xstride, dYs, ystride, dThetas, dLogML, dGrad, dAlpha, batch, dInfo, st);
    });
}

// the covariance function is a run-time argument of the kernel: the name depends on it only through "" for an unknown one
const char *matinv_ard_logml_kernel_name(int dtype, int kind, int n)
{
    if (!has_kernel_name(dtype, n) || (kind != MATINV_COV_SE && kind != MATINV_COV_MATERN52)) return "";
    return ard_tile_supports(n) ? name_ard_tile(dtype == MATINV_F64, n) : name_ard_global(dtype == MATINV_F64);
}

int matinv_ard_logml_batched_host(int dtype, int kind, int n, int ndim, const void *hXs, size_t xstride, const void *hYs, size_t ystride,
                                  const void *hThetas, void *hLogML, void *hGrad, void *hAlpha, size_t batch, int *info)
{
    int rc = ard_check_args(dtype, kind, n, ndim, hXs, xstride, hYs, ystride, hThetas, hLogML, hGrad, hAlpha, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) {
        return ard_host<decltype(t)>(kind, n, ndim, hXs, xstride, hYs, ystride, hThetas, hLogML, hGrad, hAlpha, batch, info);
    });
}

int matinv_ard_predict_batched(int dtype, int kind, int n, int ndim, int nquery, const void *dXs, size_t xstride, const void *dYs,
                               size_t ystride, const void *dThetas, const void *dXqs, size_t xqstride, void *dMean, void *dVar, size_t batch,
                               int *dInfo, void *stream)
{
    int rc = ard_predict_check_args(dtype, kind, n, ndim, nquery, dXs, xstride, dYs, ystride, dThetas, dXqs, xqstride, dMean, dVar, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return ard_predict_dispatch<decltype(t)>(kind, n, ndim, nquery, dXs, xstride, dYs, ystride, dThetas, dXqs, xqstride, dMean, dVar,
                                                 batch, dInfo, st);
    });
}

// as matinv_ard_logml_kernel_name: the covariance function is a run-time argument of the kernel
const char *matinv_ard_predict_kernel_name(int dtype, int kind, int n)
{
    if (!has_kernel_name(dtype, n) || (kind != MATINV_COV_SE && kind != MATINV_COV_MATERN52)) return "";
    return ard_predict_tile_supports(n) ? name_ard_predict_tile(dtype == MATINV_F64, n) : name_ard_predict_global(dtype == MATINV_F64);
}

int matinv_ard_predict_batched_host(int dtype, int kind, int n, int ndim, int nquery, const void *hXs, size_t xstride, const void *hYs,
                                    size_t ystride, const void *hThetas, const void *hXqs, size_t xqstride, void *hMean, void *hVar,
                                    size_t batch, int *info)
{
    int rc = ard_predict_check_args(dtype, kind, n, ndim, nquery, hXs, xstride, hYs, ystride, hThetas, hXqs, xqstride, hMean, hVar, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) {
        return ard_predict_host<decltype(t)>(kind, n, ndim, nquery, hXs, xstride, hYs, ystride, hThetas, hXqs, xqstride, hMean, hVar, batch,
                                             info);
    });
}

int matinv_sample_batched(int dtype, int n, int nquery, int nsample, const void *dBs, const void *dCs, const void *dDs, const void *dAs,
                          const void *dEs, const void *dZs, void *dY, void *dMean, void *dCov, size_t batch, int *dInfo, void *stream)
{
    int rc = sample_check_args(dtype, n, nquery, nsample, dBs, dDs, dAs, dZs, dY, dMean, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return sample_dispatch<decltype(t)>(n, nquery, nsample, dBs, dCs, dDs, dAs, dEs, dZs, dY, dMean, dCov, batch, dInfo, st);
    });
}

int matinv_sample_batched_host(int dtype, int n, int nquery, int nsample, const void *hBs, const void *hCs, const void *hDs, const void *hAs,
                               const void *hEs, const void *hZs, void *hY, void *hMean, void *hCov, size_t batch, int *info)
{
    int rc = sample_check_args(dtype, n, nquery, nsample, hBs, hDs, hAs, hZs, hY, hMean, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) {
        return sample_host<decltype(t)>(n, nquery, nsample, hBs, hCs, hDs, hAs, hEs, hZs, hY, hMean, hCov, batch, info);
    });
}

int matinv_loo_grad_batched(int dtype, int n, int nparam, const void *dBs, const void *dCs, const void *dDs, const void *dDMs, void *dGrad,
                            void *dGradC, void *dLogPL, size_t batch, int *dInfo, void *stream)
{
    int rc = loo_grad_check_args(dtype, n, nparam, dBs, dDs, dDMs, dGrad, dGradC, dLogPL, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        return loo_grad_dispatch<decltype(t)>(n, nparam, dBs, dCs, dDs, dDMs, dGrad, dGradC, dLogPL, batch, dInfo, st);
    });
}

const char *matinv_loo_grad_kernel_name(int dtype, int n)
{
    if (!has_kernel_name(dtype, n)) return "";
    return loo_grad_tile_supports(n) ? name_loo_grad_tile(dtype == MATINV_F64, n) : name_loo_grad_global(dtype == MATINV_F64);
}

int matinv_loo_grad_batched_host(int dtype, int n, int nparam, const void *hBs, const void *hCs, const void *hDs, const void *hDMs,
                                 void *hGrad, void *hGradC, void *hLogPL, size_t batch, int *info)
{
    int rc = loo_grad_check_args(dtype, n, nparam, hBs, hDs, hDMs, hGrad, hGradC, hLogPL, batch);
    if (rc != MATINV_OK || batch == 0) return rc;
    return by_dtype(dtype, [&](auto t) {
        return loo_grad_host<decltype(t)>(n, nparam, hBs, hCs, hDs, hDMs, hGrad, hGradC, hLogPL, batch, info);
    });
}

int matinv_mean_batched(int dtype, int n, const void *dAs, const void *dBs, const void *dCs, const void *dDs,
                        void *dMeans, size_t batch, int *dInfo, void *stream)
{
    return by_dtype(dtype, [&](auto t) { return gp_dispatch<decltype(t)>(n, dAs, dBs, dCs, dDs, nullptr, dMeans, batch, dInfo, stream, false); });
}

int matinv_variance_batched(int dtype, int n, const void *dAs, const void *dBs, const void *dCs, const void *dEs,
                            void *dVars, size_t batch, int *dInfo, void *stream)
{
    return by_dtype(dtype, [&](auto t) { return gp_dispatch<decltype(t)>(n, dAs, dBs, dCs, nullptr, dEs, dVars, batch, dInfo, stream, true); });
}

int matinv_mean_batched_host(int dtype, int n, const void *hAs, const void *hBs, const void *hCs, const void *hDs,
                             void *hMeans, size_t batch, int *info)
{
    return by_dtype(dtype, [&](auto t) { return gp_host<decltype(t)>(n, hAs, hBs, hCs, hDs, hMeans, batch, info, false); });
}

int matinv_variance_batched_host(int dtype, int n, const void *hAs, const void *hBs, const void *hCs, const void *hEs,
                                 void *hVars, size_t batch, int *info)
{
    return by_dtype(dtype, [&](auto t) { return gp_host<decltype(t)>(n, hAs, hBs, hCs, hEs, hVars, batch, info, true); });
}

int matinv_inverse_batched_host(int algo, int dtype, int n, const void *hA, void *hAinv, size_t batch, int *info)
{
    return by_dtype(dtype, [&](auto t) { return inverse_host<decltype(t)>(algo, n, hA, hAinv, batch, info, nullptr); });
}

// ------------------------------------------------------------------------------------------------
// The 17 reference names (include/inverse_gpu.h), fp64 under the plain name and fp32 under <name>_f32.
// `handle` is ignored exactly as the reference's hand-written kernels ignore it.
#define GJ MATINV_ALGO_GAUSS_JORDAN
#define CH MATINV_ALGO_CHOLESKY
#define KAUTO(T, n) MATINV_KERNEL_AUTO
// the reference's LU entry points promise partial pivoting (cublas getrfBatched, src/gauss/inverse_gpu.cu:24-33): where the
// MFMA tile family serves n they go straight to its pivoting kernel, whatever the Gauss-Jordan policy says
#define KLU(T, n) lu_kernel<T>(n)
#define REF_GPU(name, suffix, T, algo, logkey, KSEL)                                                                 \
    void name##suffix(void *handle, int n, T *As, T *aInvs, int batchSize)                                          \
    {                                                                                                                \
        (void)handle;                                                                                                \
        die_on(batchSize < 0 ? fail(MATINV_ERR_ARG, "negative batchSize") : inverse_host<T>(algo, n, As, aInvs,      \
               (size_t)batchSize, nullptr, logkey, KSEL(T, n)), #name);                                              \
    }
#define REF_DEV(name, suffix, T, algo, in, out, phases, KSEL)                                                        \
    void name##suffix(void *handle, int N, T **devAs, T **devAInvs, int batchSize)                                  \
    {                                                                                                                \
        (void)handle; (void)devAs; (void)devAInvs;                                                                   \
        die_on(batchSize < 0 ? fail(MATINV_ERR_ARG, "negative batchSize") : inverse_table<T>(algo, N, in, out,       \
               (size_t)batchSize, phases, KSEL(T, N)), #name);                                                       \
    }
// log keys are the reference's TIMER_INIT names for each entry point
#define REF_ALL(suffix, T)                                                                                           \
    REF_GPU(inverse_gauss_batched_gpu, suffix, T, GJ, "inverse_gauss_batched_gpu", KAUTO)             /* batched_invert.cu:99 */ \
    REF_GPU(inverse_lu_cuda_batched_gpu, suffix, T, GJ, "inverse_lu_cuda_batched_gpu", KLU)         /* gauss/inverse_gpu.cu:60 */ \
    REF_GPU(inverse_cholesky_batched_gpu, suffix, T, CH, "decompose_cholesky_batched_gpu", KAUTO)     /* inverse_cholesky_gpu.cu:397 */ \
    REF_GPU(inverse_cholesky_mm_batched_gpu, suffix, T, CH, "decompose_cholesky_mm_batched_gpu", KAUTO) /* :627 */          \
    REF_GPU(inverse_cholesky_mm2_batched_gpu, suffix, T, CH, "cholesky_mm2_batched_gpu", KAUTO)       /* :699 */            \
    REF_GPU(inverse_cholesky_stride_batched_gpu, suffix, T, CH, "inverse_cholesky_stride_batched_gpu", KAUTO) /* :189 */    \
    REF_DEV(inverse_gauss_batched_device, suffix, T, GJ, devAs, devAInvs, 7, KAUTO)   /* declared inverse_gpu.h:10, never defined there */ \
    REF_DEV(inverse_lu_cuda_batched_device, suffix, T, GJ, devAs, devAInvs, 7, KLU) /* gauss/inverse_gpu.cu:16; input kept intact here */ \
    REF_DEV(inverse_cholesky_batched_device, suffix, T, CH, devAs, devAInvs, 7, KAUTO)        /* :323 */                    \
    REF_DEV(inverse_cholesky_mm_batched_device, suffix, T, CH, devAs, devAInvs, 7, KAUTO)     /* :608 */                    \
    REF_DEV(inverse_cholesky_mm2_batched_device, suffix, T, CH, devAs, devAInvs, 7, KAUTO)    /* :693 */                    \
    /* stride family works in place on devAInvs (the *_gpu wrapper copies As there first, :213-216) */              \
    REF_DEV(inverse_cholesky_stride_batched_device, suffix, T, CH, devAInvs, devAInvs, 7, KAUTO)     /* :182 */             \
    REF_DEV(decompose_cholesky_stride_batched_device, suffix, T, CH, devAInvs, devAInvs, 1, KAUTO)   /* :96  */             \
    REF_DEV(inverse_upper_stride_batched_device, suffix, T, CH, devAInvs, devAInvs, 2, KAUTO)        /* :137 */             \
    REF_DEV(multiply_upper_stride_batched_device, suffix, T, CH, devAInvs, devAInvs, 4, KAUTO)       /* :175 */             \
    /* decompose: factor in place in devAs, strict upper triangle zeroed (:357-369, :616-624) */                    \
    REF_DEV(decompose_cholesky_batched_device, suffix, T, CH, devAs, devAs, 1, KAUTO)                                       \
    REF_DEV(decompose_cholesky_mm_batched_device, suffix, T, CH, devAs, devAs, 1, KAUTO)

REF_ALL(, double)
REF_ALL(_f32, float)

}  // extern "C"
