// logdet_tile_kernels.hip -- fp64 instantiation of the one-wavefront log-determinant / log-marginal-likelihood tile kernels
// (logdet_tile_impl.hpp) + the helpers
#include "logdet_tile_impl.hpp"

namespace matinv {

// one wavefront holds the lower triangle of up to 6 x 6 tiles plus one border tile row (n <= 96) in both precisions
bool logdet_tile_supports(int n) { return n >= 1 && n <= 96; }

template hipError_t launch_logdet_tile<double>(int, bool, const double *, size_t, const double *, const double *, double *, double *,
                                               size_t, int *, hipStream_t);

const char *name_logdet_tile(bool f64, bool border, int n)
{
    if (!logdet_tile_supports(n)) return "";
    const TileShape s = tile_shape(n);
    static thread_local char buf[64];
    snprintf(buf, sizeof buf, "matinv_logdet_tile_%s<%d, %s, %s>", f64 ? "f64" : "f32", s.nt, s.full ? "true" : "false",
             border ? "true" : "false");
    return buf;
}

}  // namespace matinv
