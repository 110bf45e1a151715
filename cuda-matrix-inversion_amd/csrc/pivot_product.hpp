// pivot_product.hpp -- the running product of an elimination's pivots as mantissa x 2^exponent, shared by the log-determinant
// kernels (logdet_tile_impl.hpp, logdet_row_kernels.hip, logdet_global_kernels.hip). The determinant itself is never formed, so
// it can neither overflow nor underflow the number format; one logarithm is taken per matrix at the end.
#pragma once
#include "common.hpp"

namespace matinv {

__device__ __forceinline__ double pp_mant(double v) { return __builtin_amdgcn_frexp_mant(v); }
__device__ __forceinline__ float pp_mant(float v) { return __builtin_amdgcn_frexp_mantf(v); }
__device__ __forceinline__ int pp_exp(double v) { return __builtin_amdgcn_frexp_exp(v); }
__device__ __forceinline__ int pp_exp(float v) { return __builtin_amdgcn_frexp_expf(v); }

// prod |pivots| = m * 2^e with m in [1/2, 1). Every multiplication rounds once (relative u), powers of two are exact: a pivot of
// exactly 1 (identity padding) changes nothing.
template <class T>
struct PivotProduct {
    T m = (T)0.5;
    int e = 1;
    // one pivot of either sign
    __device__ __forceinline__ void fold(T p)
    {
        const T t = m * pp_mant(p < 0 ? -p : p);  // in [1/4, 1)
        e += pp_exp(p) + pp_exp(t);
        m = pp_mant(t);
    }
    // the four (positive) pivots of one block step of the tile sweep
    __device__ __forceinline__ void fold(T p0, T p1, T p2, T p3)
    {
        const T f = (pp_mant(p0) * pp_mant(p1)) * (pp_mant(p2) * pp_mant(p3));
        const T t = m * f;  // in [1/32, 1): no underflow
        e += (pp_exp(p0) + pp_exp(p1)) + (pp_exp(p2) + pp_exp(p3)) + pp_exp(t);
        m = pp_mant(t);
        // the fold happens HERE: without the pin hipcc sinks the frexp chain to the end of the sweep and keeps the pivots of all 4 NT
        // block steps alive (54 spilled registers in the fp64 5 x 5 kernel), as it does with the acceptance tests (note_fail)
        asm volatile("" : "+v"(m), "+v"(e));
    }
    // log of the product. The one logarithm and e ln 2 in fp64 also for fp32, rounded once: in fp32 the rounding of e ln 2 alone would
    // be u |e ln 2| before the cancellation with log m. The mantissa is first moved to [3/4, 3/2) (exact): |log m| <= 0.41, and a
    // product in that interval (a 1 x 1 matrix near 1, say) has exponent 0 and no cancellation at all. ln 2 is taken in two pieces: the
    // upper one has 33 significant bits, so e times it is exact for |e| <= 2^20 (1024 pivots of any exponent), and the rounding error of a
    // one-piece constant -- |e| * 2.3e-17, a sixth of an ulp of the result already for a 1 x 1 matrix of 0.1 -- does not enter.
    __device__ __forceinline__ T log_value() const
    {
        const bool low = m < (T)0.75;
        const double md = low ? 2.0 * (double)m : (double)m;
        const double ed = (double)(low ? e - 1 : e);
        constexpr double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
        return (T)__builtin_fma(ed, LN2_HI, __builtin_fma(ed, LN2_LO, log(md)));
    }
};

}  // namespace matinv
