// tileq_kernels.hip -- fp64 instantiations of the pivoting MFMA tile kernel with fixed pivot rows and searched pivot columns
// (tileq_impl.hpp): one wavefront per tile column, general 128 < n <= 192 (fp64) / 256 (fp32).
#include "tileq_impl.hpp"

namespace matinv {

bool tileq_supports(bool f64, int n) { return n > 128 && n <= tileq_limit(f64); }

template hipError_t launch_gj_tileq<double>(int, BatchRef<const double>, BatchRef<double>, size_t, int *, hipStream_t, const int *, const int *,
                                          hint_t *, int *, int *);

const char *name_gj_tileq(bool f64, int n)
{
    static thread_local char buf[48];
    snprintf(buf, sizeof buf, "matinv_gj_tileqw_%s<%d, false>", f64 ? "f64" : "f32", (n + 15) / 16);
    return buf;
}

}  // namespace matinv
