// What do fp64 VALU instructions cost on gfx950 when most of their lanes are masked off?  The layout of mfma_valu_overlap.hip: one
// 512-thread workgroup per CU (96 KB of LDS keeps a second one out), waves 0-3 (one per SIMD) issue v_mfma_f64_16x16x4_f64 back to
// back, waves 4-7 (their SIMD partners) issue a dependent-free v_fmac_f64 stream (8 accumulators) under one of three EXEC masks:
//   full   all 64 lanes
//   row4   0x0001000100010001: one lane per row of 16 (the lanes PanelSolve's GATED mode keeps, tile_common.hpp)
//   row16  0x000000000000FFFF: the 16 lanes of one row
// Each stream is timed alone and together with the other (s_memtime per wave, averaged over the workgroups of the last launch). One
// variant per process, launched again and again for `seconds` so that tools/clock_sample.py can sample board power and sclk from a
// separate process:
//   hipcc --offload-arch=gfx950 -O2 tools/valu_exec_lanes.hip -o build/valu_exec_lanes
//   for v in mfma full row4 row16 mfma+full mfma+row4 mfma+row16; do timeout -k 10 60 build/valu_exec_lanes $v 2.5 || break; done
//
// Measured (MI355X, 2.5 s per variant, power and sclk = medians of the samples under load; profiles/gj64_gated_panel.txt):
//   variant      cycles per MFMA   cycles per v_fmac_f64   board power   sclk       (idle 260 W)
//   mfma              64.00                 -                687 W      2393 MHz
//   full                -                  4.26             1016 W      2390 MHz
//   row4                -                  4.27              504 W      2382 MHz
//   row16               -                  4.27              609 W      2383 MHz
//   mfma+full         64.00                8.17              793 W      2370 MHz
//   mfma+row4         64.00                8.05              622 W      2379 MHz
//   mfma+row16        64.00                7.90              664 W      2393 MHz
// A masked lane saves no issue cycle -- the instruction takes its four passes whatever EXEC holds, and next to an MFMA wave it gets every
// other slot either way -- but it saves power: above idle the full stream draws 756 W, the same stream with 4 of 64 lanes 244 W (a third),
// with 16 lanes 349 W. A kernel that runs at the power cap turns that into clock.
#include <hip/hip_runtime.h>
#include <chrono>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
typedef double v4d __attribute__((ext_vector_type(4)));
#define REP8(x) x x x x x x x x
constexpr int BLOCKS = 256, ITERS = 2048;
constexpr int FMA_PER_ITER = 64, FMA_ITERS = ITERS * 4, MFMA_PER_ITER = 32;

// EXEC is narrowed and restored inside every asm block (64 FMAs): no compiler-generated instruction runs under the narrowed mask
#define FMA8                                                                                                                       \
    "v_fmac_f64_e32 %0, %9, %9\n\tv_fmac_f64_e32 %1, %9, %9\n\tv_fmac_f64_e32 %2, %9, %9\n\tv_fmac_f64_e32 %3, %9, %9\n\t"            \
    "v_fmac_f64_e32 %4, %9, %9\n\tv_fmac_f64_e32 %5, %9, %9\n\tv_fmac_f64_e32 %6, %9, %9\n\tv_fmac_f64_e32 %7, %9, %9\n\t"

__global__ __launch_bounds__(512) void k(double *out, long long *cyc, double seed, int run_mfma, int run_fma, unsigned long long lanes)
{
    __shared__ double pad[12 * 1024];  // 96 KB: one workgroup per CU
    const int wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) pad[0] = seed;
    __syncthreads();
    double r = 0;
    long long t0 = 0, t1 = 0;
    if (wave < 4) {
        if (run_mfma) {
            v4d c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0;
            const double a = seed + threadIdx.x, b = 1e-9 * a;
            t0 = __builtin_amdgcn_s_memtime();
            for (int it = 0; it < ITERS; ++it) {
                REP8(c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c0, 0, 0, 0); c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c1, 0, 0, 0);)
                REP8(c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c2, 0, 0, 0); c3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c3, 0, 0, 0);)
            }
            t1 = __builtin_amdgcn_s_memtime();
            r = c0[0] + c1[1] + c2[2] + c3[3];
        }
    } else if (run_fma) {
        double a0 = seed + threadIdx.x, a1 = a0 * 1.1, a2 = a0 * 1.2, a3 = a0 * 1.3, a4 = a0 * 1.4, a5 = a0 * 1.5, a6 = a0 * 1.6, a7 = a0 * 1.7;
        const double m = 1e-9 * seed;
        unsigned long long save;
        t0 = __builtin_amdgcn_s_memtime();
        for (int it = 0; it < FMA_ITERS; ++it) {
            asm volatile("s_and_saveexec_b64 %8, %10\n\t" REP8(FMA8) "s_mov_b64 exec, %8"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7), "=&s"(save)
                         : "v"(m), "s"(lanes)
                         : "scc");
        }
        t1 = __builtin_amdgcn_s_memtime();
        r = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
    }
    out[(size_t)blockIdx.x * 512 + threadIdx.x] = r + pad[0];
    if ((threadIdx.x & 63) == 0) cyc[blockIdx.x * 8 + wave] = t1 - t0;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        printf("usage: %s mfma|full|row4|row16|mfma+full|mfma+row4|mfma+row16 [seconds]\n", argv[0]);
        return 2;
    }
    const char *v = argv[1];
    const double seconds = argc > 2 ? atof(argv[2]) : 2.5;
    const int run_mfma = strncmp(v, "mfma", 4) == 0;
    const char *p = run_mfma ? (v[4] == '+' ? v + 5 : "") : v;
    unsigned long long lanes = 0;
    if (!strcmp(p, "full")) lanes = ~0ULL;
    else if (!strcmp(p, "row4")) lanes = 0x0001000100010001ULL;
    else if (!strcmp(p, "row16")) lanes = 0xFFFFULL;
    else if (*p) { printf("unknown variant %s\n", v); return 2; }
    const int run_fma = lanes != 0;
    double *o = nullptr;
    long long *c = nullptr;
    static long long h[BLOCKS * 8];
    if (hipMalloc(&o, (size_t)BLOCKS * 512 * 8) != hipSuccess || hipMalloc(&c, sizeof h) != hipSuccess) { printf("alloc failed\n"); return 1; }
    int launches = 0;
    const auto w0 = std::chrono::steady_clock::now();
    double wall = 0;
    do {
        for (int i = 0; i < 8; ++i) hipLaunchKernelGGL(k, dim3(BLOCKS), dim3(512), 0, 0, o, c, 1.0, run_mfma, run_fma, lanes);
        launches += 8;
        if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 1; }
        wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
    } while (wall < seconds);
    if (hipMemcpy(h, c, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 1; }
    double sm = 0, sp = 0;
    for (int b = 0; b < BLOCKS; ++b) { sm += h[b * 8 + 0]; sp += h[b * 8 + 4]; }
    printf("%-11s lanes %016llx  mfma wave %9.0f cyc (%6.2f per MFMA)  fma wave %9.0f cyc (%5.2f per v_fmac_f64)  %d launches, %.3f ms each\n", v, lanes,
           sm / BLOCKS, sm / BLOCKS / ((double)ITERS * MFMA_PER_ITER), sp / BLOCKS, sp / BLOCKS / ((double)FMA_ITERS * FMA_PER_ITER), launches,
           1e3 * wall / launches);
    return 0;
}
