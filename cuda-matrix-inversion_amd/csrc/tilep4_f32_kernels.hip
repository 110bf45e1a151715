// tilep4_f32_kernels.hip -- fp32 instantiations of the three- / four-wavefront pivoting MFMA tile kernels (tilep4_impl.hpp).
#include "tilep4_impl.hpp"

namespace matinv {

template hipError_t launch_gj_tilep4<float>(int, BatchRef<const float>, BatchRef<float>, size_t, int *, hipStream_t);
template hipError_t launch_gj_tilep4_worklist<float>(int, BatchRef<const float>, BatchRef<float>, size_t, const int *, const int *, int *,
                                                     int *, int *, hipStream_t, hint_t *, bool);

}  // namespace matinv
