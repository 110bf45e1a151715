// tile_gj_f32_kernels.hip -- fp32 natural-order Gauss-Jordan MFMA tile kernels, n <= 64, with their screening pass (tile_impl.hpp).
#include "tile_impl.hpp"

namespace matinv {

template hipError_t launch_gj_tile<float>(int, BatchRef<const float>, BatchRef<float>, size_t, int *, hipStream_t);

}  // namespace matinv
