// multi_target_grad_tile_kernels.hip -- fp64 instantiation of the one-wavefront multi-target gradient tile kernels
// (multi_target_grad_tile_impl.hpp) + the helpers
#include "multi_target_grad_tile_impl.hpp"

namespace matinv {

// one wavefront holds the lower triangle of up to 6 x 6 tiles (n <= 96) in both precisions
bool multi_target_grad_tile_supports(int n) { return n >= 1 && n <= 96; }

template hipError_t launch_multi_target_grad_tile<double>(int, int, int, const double *, const double *, const double *, const double *,
                                                          double *, double *, double *, double *, size_t, int *, hipStream_t);

// the gradient form of the multi-target kernel of the same tile shape: its name with a third to an eleventh template argument
const char *name_multi_target_grad_tile(bool f64, int n)
{
    if (!multi_target_grad_tile_supports(n)) return "";
    const TileShape s = tile_shape(n);
    static thread_local char buf[120];
    snprintf(buf, sizeof buf, "matinv_spd_tile_%s<%d, %s, true, true, true, true, true, true, true, true, true>", f64 ? "f64" : "f32", s.nt,
             s.full ? "true" : "false");
    return buf;
}

}  // namespace matinv
