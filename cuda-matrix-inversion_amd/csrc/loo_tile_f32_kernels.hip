// loo_tile_f32_kernels.hip -- fp32 instantiation of the one-wavefront leave-one-out tile kernels (loo_tile_impl.hpp); a translation
// unit of its own so that the two precisions compile in parallel
#include "loo_tile_impl.hpp"

namespace matinv {

template hipError_t launch_loo_tile<float>(int, const float *, const float *, const float *, float *, float *, float *, size_t, int *,
                                           hipStream_t);

}  // namespace matinv
