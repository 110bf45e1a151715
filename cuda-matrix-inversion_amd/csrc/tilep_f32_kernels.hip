// tilep_f32_kernels.hip -- fp32 instantiations of the pivoting MFMA tile kernels (tilep_impl.hpp).
#include "tilep_impl.hpp"

namespace matinv {

template hipError_t launch_gj_tilep<float>(int, BatchRef<const float>, BatchRef<float>, size_t, int *, hipStream_t);
template hipError_t launch_gj_tilep_worklist<float>(int, BatchRef<const float>, BatchRef<float>, size_t, const int *, const int *, int *,
                                                    int *, int *, hipStream_t, hint_t *, bool, const int *, hint_t *);

}  // namespace matinv
