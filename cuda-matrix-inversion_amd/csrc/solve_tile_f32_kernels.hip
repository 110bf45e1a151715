// solve_tile_f32_kernels.hip -- fp32 fused bordered solve kernels, 16 < n <= 64, nrhs <= 16 (solve_tile_impl.hpp).
#include "solve_tile_impl.hpp"

namespace matinv {

template hipError_t launch_solve_tile<float>(int, int, int, BatchRef<const float>, BatchRef<const float>, BatchRef<float>, size_t, int *,
                                             hipStream_t);

}  // namespace matinv
