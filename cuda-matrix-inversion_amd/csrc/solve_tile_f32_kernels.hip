// solve_tile_f32_kernels.hip -- fp32 fused bordered solve kernels, 16 < n <= 64, nrhs <= 16 (solve_tile_impl.hpp). Three waves per SIMD:
// with four (128 registers) the 4 x 4-tile instantiation spills the border.
#include "solve_tile_impl.hpp"

namespace matinv {

template <int NT, bool FULL, bool SPD>
__global__ __launch_bounds__(64, 3) void matinv_solve_tile_f32(BatchRef<const float> A, BatchRef<const float> B, BatchRef<float> X,
                                                               int *info, int n, int nrhs, unsigned batch, int *work_count,
                                                               int *work_list)
{
    __shared__ __attribute__((aligned(16))) float panel[16 * (NT + 1) * 4];  // [row][4 pivot columns], border rows last
    solve_tile_body<float, NT, FULL, SPD>(A, B, X, info, n, nrhs, batch, work_count, work_list, panel);
}

template <>
hipError_t launch_solve_tile<float>(int algo, int n, int nrhs, BatchRef<const float> A, BatchRef<const float> B, BatchRef<float> X,
                                     size_t batch, int *info, hipStream_t stream)
{
    auto launch = [&](int nt, bool full, bool spd, unsigned grid, auto... args) {
#define SOLVE_LAUNCH(NT_, FULL_, SPD_) \
    hipLaunchKernelGGL((matinv_solve_tile_f32<NT_, FULL_, SPD_>), dim3(grid), dim3(64), 0, stream, args...)
#define SOLVE_LAUNCH_NT(NT_)                                                  \
    do {                                                                      \
        if (full && spd) SOLVE_LAUNCH(NT_, true, true);                       \
        else if (full) SOLVE_LAUNCH(NT_, true, false);                        \
        else if (spd) SOLVE_LAUNCH(NT_, false, true);                         \
        else SOLVE_LAUNCH(NT_, false, false);                                 \
    } while (0)
        switch (nt) {
        case 2: SOLVE_LAUNCH_NT(2); break;
        case 3: SOLVE_LAUNCH_NT(3); break;
        default: SOLVE_LAUNCH_NT(4); break;
        }
#undef SOLVE_LAUNCH_NT
#undef SOLVE_LAUNCH
    };
    return launch_solve_tile_impl<float>(algo, n, nrhs, A, B, X, batch, info, stream, launch);
}

}  // namespace matinv
