// tile_gj_kernels.hip -- fp64 natural-order Gauss-Jordan MFMA tile kernels, n <= 64, with their screening pass (tile_impl.hpp).
// tools/build_ldst_variant.sh rebuilds this translation unit alone: these kernels and launch_gj_tile<double> live here only.
#include "tile_impl.hpp"

namespace matinv {

template hipError_t launch_gj_tile<double>(int, BatchRef<const double>, BatchRef<double>, size_t, int *, hipStream_t);

}  // namespace matinv
