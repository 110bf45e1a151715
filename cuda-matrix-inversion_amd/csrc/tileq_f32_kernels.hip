// tileq_f32_kernels.hip -- fp32 instantiations of the pivoting MFMA tile kernel with fixed pivot rows and searched pivot
// columns (tileq_impl.hpp).
#include "tileq_impl.hpp"

namespace matinv {

template hipError_t launch_gj_tileq<float>(int, BatchRef<const float>, BatchRef<float>, size_t, int *, hipStream_t, const int *, const int *,
                                         hint_t *, int *, int *);

}  // namespace matinv
