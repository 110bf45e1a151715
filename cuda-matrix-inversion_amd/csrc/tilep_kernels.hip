// tilep_kernels.hip -- fp64 instantiations of the pivoting MFMA tile kernels (tilep_impl.hpp) and the family's helpers.
#include "tilep_impl.hpp"

namespace matinv {

bool tilep_supports(int n) { return n >= 1 && n <= 128; }

template hipError_t launch_gj_tilep<double>(int, BatchRef<const double>, BatchRef<double>, size_t, int *, hipStream_t);
template hipError_t launch_gj_tilep_worklist<double>(int, BatchRef<const double>, BatchRef<double>, size_t, const int *, const int *, int *,
                                                     int *, int *, hipStream_t, hint_t *, bool, const int *, hint_t *);

const char *name_gj_tilep(bool f64, int n)
{
    if (n > 64) return name_gj_tilep4(f64, n);
    const TileShape s = tile_shape(n);
    static thread_local char buf[48];
    snprintf(buf, sizeof buf, "matinv_gj_tilep_%s<%d, %s>", f64 ? "f64" : "f32", s.nt, s.full ? "true" : "false");
    return buf;
}

}  // namespace matinv
