// tile_kernels.hip -- fp64 symmetric sweeps of the one-wavefront MFMA tile family (tile_impl.hpp) up to 6 x 6 lower tiles: the Cholesky
// entry point (launch_spd_tile<double>) and the fused mean / variance (launch_gp_spd_tile<double>); and the family's non-template
// helpers: the grid rounds, the Gauss-Jordan policy with its hint slots, the size limits and the kernel names.
#include "tile_impl.hpp"

namespace matinv {

// r03: ONE wavefront per matrix beyond what 256 registers hold. A gfx950 wave may own up to 512 registers -- 256 VGPRs + 256
// AGPRs, one file, and MFMA accumulates in AGPRs directly -- when its kernel asks for one wave per SIMD: hipcc then keeps the
// accumulator tiles in AGPRs (fp64 7 x 7 lower tiles: 190 VGPRs + 224 AGPRs, no scratch). Four matrices per CU, no workgroup barrier,
// no panel solve repeated per wave; r01/r02 stopped the one-wave kernels at 256 registers (two waves per SIMD) and went to several
// wavefronts per matrix from there.

// Measured at 100 k x 64^2 f64: 1 / 4 / 16 / 64 rounds -> 1.631 / 1.600 / 1.579 / 1.570 ms per launch: the hardware
// dispatcher balances better than a static stride does, so the grids are (nearly) one workgroup per matrix and the stride
// loop only matters for batches beyond 64 rounds.
unsigned tile_grid_rounds()
{
    static const unsigned rounds = []() {
        const char *s = getenv("MATINV_TILE_GRID_MULT");
        const int v = s && *s ? atoi(s) : 64;
        return (unsigned)(v < 1 ? 1 : v);
    }();
    return rounds;
}

// ---- natural order or pivot search? -------------------------------------------------------------------------------------
// The verified-natural-order kernel is the fast path for diagonally dominant / SPD batches (0.50 of HBM at 64 x 64); a matrix
// that fails its acceptance test is redone by the pivoting kernel in the same stream. Three policies (matinv_set_gj_policy,
// MATINV_GJ_POLICY=natural|pivot|adaptive):
//   NATURAL_FIRST (default since r03): every launch runs the natural-order kernel, rejects go to the pivoting kernel. What a
//       matrix's result is depends on that matrix alone -- no launch history, no batch mates: the same call gives the same
//       bits again, and a sharded batch the bits of the single launch. A batch of GENERAL matrices pays both kernels.
//   PIVOT: every launch goes straight to the pivoting kernel (equally deterministic; what the reference's LU entry points,
//       inverse_lu_cuda_batched_*, take: partial pivoting is their contract, src/gauss/inverse_gpu.cu:16-58).
//   ADAPTIVE (r02 behaviour, opt-in): per (device, dtype, tile count) the launcher remembers how the LAST natural-order launch
//       that has completed went -- (rejected, batch) come back as ONE 8-byte store of the work-list kernel into pinned host
//       memory, never waited for -- and sends a batch straight to the pivoting kernel while at least a quarter of that launch
//       was rejected; every 32nd launch in that state probes the natural order again. Fastest for callers that alternate
//       rarely; a matrix that the natural-order kernel would accept although partial pivoting would move rows gets the
//       pivoting kernel's bits or the natural ones depending on what ran before.
// All of the state is per device and atomic: host threads driving different devices (or one device) do not race on it.
namespace {
constexpr int kMaxDevices = 16, kSlotsPerDevice = 64;
struct HintSlot {
    std::atomic<unsigned long long> pair;       // (batch << 32) | rejected of the last completed natural-order launch: device store
    std::atomic<unsigned> launches_in_pivot_mode;
};
HintSlot *hint_slots()
{
    static HintSlot *slots = []() -> HintSlot * {
        void *p = nullptr;
        if (hipHostMalloc(&p, sizeof(HintSlot) * kMaxDevices * kSlotsPerDevice, hipHostMallocPortable) != hipSuccess) return nullptr;
        memset(p, 0, sizeof(HintSlot) * kMaxDevices * kSlotsPerDevice);
        return static_cast<HintSlot *>(p);
    }();
    return slots;
}
std::atomic<int> g_policy{-1};  // -1: not read from the environment yet
std::atomic<unsigned long long> g_natural_launches{0}, g_pivot_launches{0};
std::atomic<int> g_last_slot{0};
int slot_index(bool f64, int nt)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    return (dev % kMaxDevices) * kSlotsPerDevice + (f64 ? 32 : 0) + (nt & 31);
}
}  // namespace

int gj_policy()
{
    int v = g_policy.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *s = getenv("MATINV_GJ_POLICY");
        v = MATINV_GJ_NATURAL_FIRST;
        if (s && !strcmp(s, "pivot")) v = MATINV_GJ_PIVOT;
        else if (s && !strcmp(s, "adaptive")) v = MATINV_GJ_ADAPTIVE;
        int expected = -1;
        if (!g_policy.compare_exchange_strong(expected, v)) v = expected;  // somebody set it meanwhile
    }
    return v;
}

int set_gj_policy(int policy)
{
    const int old = gj_policy();
    g_policy.store(policy, std::memory_order_relaxed);
    return old;
}

bool tile_policy_use_pivot(bool f64, int nt)
{
    const int pol = gj_policy();
    bool pivot = pol == MATINV_GJ_PIVOT;
    if (pol == MATINV_GJ_ADAPTIVE) {
        HintSlot *h = hint_slots();
        const int idx = slot_index(f64, nt);
        g_last_slot.store(idx, std::memory_order_relaxed);
        if (h) {
            const unsigned long long pr = h[idx].pair.load(std::memory_order_relaxed);
            const unsigned long long batch = pr >> 32, rejected = pr & 0xffffffffull;
            if (batch > 0 && 4ull * rejected >= batch)
                pivot = ((h[idx].launches_in_pivot_mode.fetch_add(1, std::memory_order_relaxed) + 1) % 32u) != 0;  // every 32nd probes
        }
    }
    (pivot ? g_pivot_launches : g_natural_launches).fetch_add(1, std::memory_order_relaxed);
    return pivot;
}

// before a natural-order launch: where the work-list kernel that follows it in the stream stores (batch << 32) | rejected
// (pinned host memory, one 8-byte store, never waited for), or nullptr when nobody reads it
hint_t *tile_policy_record(bool f64, int nt, size_t batch)
{
    (void)batch;
    if (gj_policy() == MATINV_GJ_PIVOT) return nullptr;
    HintSlot *h = hint_slots();
    if (!h) return nullptr;
    static_assert(sizeof(std::atomic<unsigned long long>) == sizeof(hint_t), "the device stores into the atomic's storage");
    return reinterpret_cast<hint_t *>(&h[slot_index(f64, nt)].pair);
}

// NATURAL_FIRST: run the screening kernel (gj_tile_screen_body) in front of the natural-order kernel? Yes while the last completed
// natural-order launch of this class rejected at least a quarter of its batch. It changes what a launch costs, never what it
// computes. MATINV_TILE_SCREEN=0 / 1: never / always (tests, A/B).
bool tile_policy_use_screen(bool f64, int nt)
{
    static const int forced = []() {
        const char *s = getenv("MATINV_TILE_SCREEN");
        return !s || !*s ? -1 : (*s == '0' ? 0 : 1);
    }();
    if (forced >= 0) return forced == 1;
    if (gj_policy() != MATINV_GJ_NATURAL_FIRST) return false;
    HintSlot *h = hint_slots();
    if (!h) return false;
    const unsigned long long pr = h[slot_index(f64, nt)].pair.load(std::memory_order_relaxed);
    const unsigned long long batch = pr >> 32, rejected = pr & 0xffffffffull;
    return batch > 0 && 4ull * rejected >= batch;
}

// ---- 64 x 64 fp64, unscreened: symmetric-only kernel in front, or the two-arm kernel alone? (launch_gj_tile_natural) ------------
// The FRONT route pays one more small launch and, for every matrix that is not symmetric, a second set of loads; the DIRECT route
// runs a symmetric matrix at two waves per SIMD instead of three. The choice follows launch history like the screening pass does and
// never changes a result: FRONT unless the last front launch of this device and tile count that has COMPLETED found at least a
// quarter of its batch not symmetric -- that count comes back like the reject hint, one 8-byte store of the work-list kernel that
// ends the chain into pinned host memory, never waited for -- and in that state every 32nd launch probes the front route again.
namespace {
struct FrontSlot {
    std::atomic<unsigned long long> pair;  // (batch << 32) | not symmetric, of the last completed front launch: device store
    std::atomic<unsigned> launches_in_direct_mode;
};
FrontSlot *front_slots()
{
    static FrontSlot *slots = []() -> FrontSlot * {
        void *p = nullptr;
        if (hipHostMalloc(&p, sizeof(FrontSlot) * kMaxDevices * kSlotsPerDevice, hipHostMallocPortable) != hipSuccess) return nullptr;
        memset(p, 0, sizeof(FrontSlot) * kMaxDevices * kSlotsPerDevice);
        return static_cast<FrontSlot *>(p);
    }();
    return slots;
}
std::atomic<unsigned long long> g_front_launches{0}, g_direct_launches{0};
std::atomic<int> g_last_front_slot{0};
}  // namespace

bool tile_policy_use_sym_front(int nt)
{
    FrontSlot *h = front_slots();
    bool front = h != nullptr;  // without the slots nobody would ever learn that a batch is not symmetric
    if (h) {
        const int idx = slot_index(true, nt);
        g_last_front_slot.store(idx, std::memory_order_relaxed);
        const unsigned long long pr = h[idx].pair.load(std::memory_order_relaxed);
        const unsigned long long batch = pr >> 32, notsym = pr & 0xffffffffull;
        if (batch > 0 && 4ull * notsym >= batch)
            front = ((h[idx].launches_in_direct_mode.fetch_add(1, std::memory_order_relaxed) + 1) % 32u) == 0;  // every 32nd probes
        else
            h[idx].launches_in_direct_mode.store(0, std::memory_order_relaxed);
    }
    (front ? g_front_launches : g_direct_launches).fetch_add(1, std::memory_order_relaxed);
    return front;
}

// before a front launch: where the work-list kernel behind it stores (batch << 32) | not symmetric
hint_t *tile_policy_record_sym_front(int nt)
{
    FrontSlot *h = front_slots();
    static_assert(sizeof(std::atomic<unsigned long long>) == sizeof(hint_t), "the device stores into the atomic's storage");
    return h ? reinterpret_cast<hint_t *>(&h[slot_index(true, nt)].pair) : nullptr;
}

SymFrontStats sym_front_stats()
{
    FrontSlot *h = front_slots();
    SymFrontStats t{g_front_launches.load(), g_direct_launches.load(), 0, 0};
    if (h) {
        const unsigned long long pr = h[g_last_front_slot.load()].pair.load(std::memory_order_relaxed);
        t.last_not_symmetric = pr & 0xffffffffull;
        t.last_batch = pr >> 32;
    }
    return t;
}

TileStats tile_stats()
{
    HintSlot *h = hint_slots();
    TileStats t{g_natural_launches.load(), g_pivot_launches.load(), 0, 0};
    if (h) {
        const unsigned long long pr = h[g_last_slot.load()].pair.load(std::memory_order_relaxed);
        t.last_rejected = pr & 0xffffffffull;
        t.last_batch = pr >> 32;
    }
    return t;
}

template <class T>
bool tile_family_supports(int n) { return n >= 1 && n <= (sizeof(T) == 8 ? 192 : 256); }  // 64 < n: tile4_kernels.hip (up to 12 x 12 tiles in fp64)
template <class T>
bool spd_tile_supports(int n) { return n >= 1 && n <= (sizeof(T) == 8 ? 192 : 256); }
template bool tile_family_supports<double>(int);
template bool tile_family_supports<float>(int);
template bool spd_tile_supports<double>(int);
template bool spd_tile_supports<float>(int);

// largest n the ONE-wavefront symmetric sweep takes: fp64 7 x 7 lower tiles (224 accumulator registers, VGPRs + AGPRs, one wave
// per SIMD); fp32 10 x 10 (55 tiles = 220 registers, one wave per SIMD; 11 x 11 = 264: 2 KB of scratch per lane)
int spd_onewave_max(bool f64) { return f64 ? 112 : 160; }
bool gp_spd_tile_supports(bool f64, int n) { return n > (f64 ? 80 : 96) && n <= spd_onewave_max(f64); }

// the tile count picks the instantiation (run-time n only): launch_gp_spd_tile and the two wide translation units
const char *name_gp_spd_tile(bool f64, int n)
{
    static thread_local char buf[48];
    snprintf(buf, sizeof buf, "matinv_gp_spd_tile_%s<%d>", f64 ? "f64" : "f32", (n + 15) / 16);
    return buf;
}

template hipError_t launch_gp_spd_tile<double>(int, const double *, const double *, const double *, const double *, const double *, double *,
                                               size_t, int *, hipStream_t);

template <>
hipError_t launch_spd_tile<double>(int n, BatchRef<const double> A, BatchRef<double> X, size_t batch, int *info, hipStream_t stream)
{
    if (!spd_tile_supports<double>(n)) return hipErrorInvalidValue;
    // one wavefront holds the lower triangle up to 6 x 6 tiles in 256 registers (two waves per SIMD) and 7 x 7 in VGPRs + AGPRs
    // (one wave per SIMD, r03; before that 7 x 7 spilled: 5.8e6 inv/s at 112 x 112 against 9.9e6 on four wavefronts)
    if (spd_tile2_supports(true, n)) return launch_spd_tile2(n, A, X, batch, info, stream);  // 112 < n <= 192: two / three waves, lower tiles
    if (batch == 0) return hipSuccess;
    return with_scratch_ints(batch + 1, 1, stream, [&](int *ws) {
        const TileShape s = spd_tile_shape(true, n);
        const unsigned grid = tile_grid(batch, 12u), b = (unsigned)batch;
        hipError_t e = hipSuccess;
        if (s.nt <= 6)
            with_tile<1, 6>(s, [&](auto NT, auto FULL) {
                hipLaunchKernelGGL((matinv_spd_tile_f64<NT, FULL>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1);
            });
        else
            e = enqueue_spd_tile_wide_f64(n, A, X, grid, b, info, ws, stream);  // 7 x 7: spd_wide_f64_kernels.hip
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = launch_chol_lds_worklist<double>(n, A, X, ws, ws + 1, info, stream);
        return e;
    });
}

const char *name_spd_tile(bool f64, int n)
{
    if (spd_tile2_supports(f64, n)) return name_spd_tile2(false, n);
    if (n > spd_onewave_max(f64)) return name_tile4(f64, true, n);
    const TileShape s = spd_tile_shape(f64, n);
    static thread_local char buf[48];
    snprintf(buf, sizeof buf, "matinv_spd_tile_%s<%d, %s>", f64 ? "f64" : "f32", s.nt, s.full ? "true" : "false");
    return buf;
}

const char *name_gj_tile(bool f64, int n)
{
    if (n > 64) return name_tile4(f64, false, n);
    if (rowlane2_supports(n)) return name_gj_rowlane2(f64, n);
    // the instantiation the launcher takes without the screening pass (the default EARLY = false left out)
    const TileShape s = tile_shape(n);
    static thread_local char buf[48];
    snprintf(buf, sizeof buf, "matinv_gj_tile_%s<%d, %s, true>", f64 ? "f64" : "f32", s.nt, s.full ? "true" : "false");
    return buf;
}

}  // namespace matinv
