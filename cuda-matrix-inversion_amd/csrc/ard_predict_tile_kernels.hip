// ard_predict_tile_kernels.hip -- fp64 instantiation of the one-wavefront tile kernels of GP prediction from coordinates
// (ard_predict_tile_impl.hpp) + the helpers
#include "ard_predict_tile_impl.hpp"

namespace matinv {

// the sizes of the ARD forms whose generation and sweep these kernels run
bool ard_predict_tile_supports(int n) { return ard_tile_supports(n); }

template hipError_t launch_ard_predict_tile<double>(int, int, int, int, const double *, size_t, const double *, size_t, const double *,
                                                    const double *, size_t, double *, double *, size_t, int *, hipStream_t);

// the bordered log-determinant kernel's name with a fourth template argument
const char *name_ard_predict_tile(bool f64, int n)
{
    if (!ard_predict_tile_supports(n)) return "";
    const TileShape s = tile_shape(n);
    static thread_local char buf[64];
    snprintf(buf, sizeof buf, "matinv_logdet_tile_%s<%d, %s, true, true>", f64 ? "f64" : "f32", s.nt, s.full ? "true" : "false");
    return buf;
}

}  // namespace matinv
