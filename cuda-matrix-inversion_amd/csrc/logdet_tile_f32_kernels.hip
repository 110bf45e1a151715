// logdet_tile_f32_kernels.hip -- fp32 instantiation of the one-wavefront log-determinant / log-marginal-likelihood tile
// kernels (logdet_tile_impl.hpp); a translation unit of its own so that the two precisions compile in parallel
#include "logdet_tile_impl.hpp"

namespace matinv {

template hipError_t launch_logdet_tile<float>(int, bool, const float *, size_t, const float *, const float *, float *, float *, size_t,
                                              int *, hipStream_t);

}  // namespace matinv
