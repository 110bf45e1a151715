// gp_tile_kernels.hip -- fp64 instantiation of the one-wavefront fused pipeline kernels (gp_tile_impl.hpp) + the helpers
#include "gp_tile_impl.hpp"

namespace matinv {

// one wavefront holds the bordered lower triangle of up to 7 x 7 tiles: fp32 n <= 96. In fp64 the last size spills 292 B per lane and the
// SPD sweep with the bilinear form folded out of the accumulators (gp_spd_tile_supports) takes 80 < n <= 96: 6 x 6 tiles are not built.
// n <= 16 belongs to the rowlane kernel: the one-tile instantiation is not built either
bool gp_tile_supports(bool f64, int n) { return n > 16 && n <= (f64 ? 80 : 96); }

template hipError_t launch_gp_tile<double>(int, const double *, const double *, const double *, const double *,
                                           const double *, double *, size_t, int *, hipStream_t);

const char *name_gp_tile(bool f64, int n)
{
    const TileShape s = tile_shape(n);
    static thread_local char buf[48];
    snprintf(buf, sizeof buf, "matinv_gp_tile_%s<%d, %s>", f64 ? "f64" : "f32", s.nt, s.full ? "true" : "false");
    return buf;
}

}  // namespace matinv
