// ard_tile_kernels.hip -- fp64 instantiation of the one-wavefront tile kernels of the GP log marginal likelihood from coordinates
// (ard_tile_impl.hpp) + the helpers
#include "ard_tile_impl.hpp"

namespace matinv {

// the sizes of the other GP tile forms: one wavefront holds the lower triangle of up to 6 x 6 tiles (n <= 96) in both precisions
bool ard_tile_supports(int n) { return trend_loo_tile_supports(n); }

template hipError_t launch_ard_tile<double>(int, int, int, const double *, size_t, const double *, size_t, const double *, double *, double *,
                                            double *, size_t, int *, hipStream_t);

// the ARD form of the SPD inversion kernel of the same tile shape: its name with a third to a fifteenth template argument
const char *name_ard_tile(bool f64, int n)
{
    if (!ard_tile_supports(n)) return "";
    const TileShape s = tile_shape(n);
    static thread_local char buf[152];
    snprintf(buf, sizeof buf, "matinv_spd_tile_%s<%d, %s, true, true, true, true, true, true, true, true, true, true, true, true, true>",
             f64 ? "f64" : "f32", s.nt, s.full ? "true" : "false");
    return buf;
}

}  // namespace matinv
