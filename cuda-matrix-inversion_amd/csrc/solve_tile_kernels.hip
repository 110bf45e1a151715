// solve_tile_kernels.hip -- fp64 fused bordered solve kernels, 16 < n <= 64, nrhs <= 16 (solve_tile_impl.hpp).
#include "solve_tile_impl.hpp"

namespace matinv {

template hipError_t launch_solve_tile<double>(int, int, int, BatchRef<const double>, BatchRef<const double>, BatchRef<double>, size_t, int *,
                                              hipStream_t);

}  // namespace matinv
