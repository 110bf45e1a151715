// tilep4_kernels.hip -- fp64 instantiations of the three- / four-wavefront pivoting MFMA tile kernels (tilep4_impl.hpp), general
// 64 < n <= 128.
// Measured against this kernel and not kept (r02 - r04; DESIGN.md, appendix "experiments that lost"): one wavefront per tile column
// with one searching wave and a barrier every 4 columns, the same with one barrier per tile column (16 pivots), the ONE-wavefront
// pivoting kernel on VGPRs + AGPRs for 64 < n <= 96, four wavefronts also at 5 x 5 / 6 x 6 tiles, and -- r04 -- the kernel with fixed
// pivot rows and searched pivot columns that now serves 128 < n (tileq_impl.hpp): at these sizes within 2 - 7 % of this one in fp64,
// 1.7 x slower in fp32.
#include "tilep4_impl.hpp"

namespace matinv {

template hipError_t launch_gj_tilep4<double>(int, BatchRef<const double>, BatchRef<double>, size_t, int *, hipStream_t);
template hipError_t launch_gj_tilep4_worklist<double>(int, BatchRef<const double>, BatchRef<double>, size_t, const int *, const int *, int *,
                                                      int *, int *, hipStream_t, hint_t *, bool);

const char *name_gj_tilep4(bool f64, int n)
{
    const TileShape s = tile_shape(n);
    static thread_local char buf[48];
    snprintf(buf, sizeof buf, "matinv_gj_tilep%d_%s<%d, %s>", tilep4_waves(s.nt), f64 ? "f64" : "f32", s.nt, s.full ? "true" : "false");
    return buf;
}

}  // namespace matinv
