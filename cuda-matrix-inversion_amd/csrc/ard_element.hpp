// ard_element.hpp -- the covariance element of the ARD kernels (ard_tile_impl.hpp, the ARD form of matinv_chol_global): ONE function of
// (s, kind) gives phi and psi = -2 phi', and every place that needs an element of M or of a derivative matrix calls it, with contraction
// off, so a regenerated element has the bits of the generated one.
#pragma once
#include "../../include/matinv.h"
#include "common.hpp"

namespace matinv {

// A 64-bit constant of the exponential below, pinned into a scalar register pair where it is used: as a literal hipcc builds it in a
// vector register pair at the top of the kernel, keeps it there across the whole sweep and spills it to scratch beside the accumulators
// (the fp64 2 x 2 form: 39 registers of such constants with exp() of the device library).
__device__ __forceinline__ double ard_const(double v)
{
    asm volatile("" : "+s"(v));
    return v;
}
__device__ __forceinline__ float ard_const(float v) { return v; }  // a 32-bit literal is an operand of the instruction

// exp(x) by Cody-Waite reduction x = n ln 2 + r, |r| <= ln 2 / 2, and the Taylor polynomial of exp(r) in Horner form (degree 13: the
// remainder is below 4e-18; n ln2_hi is exact for |n| < 2^20). Error below 2 ulp: 1/2 from r, 1 from the last two Horner steps, the rest
// from the polynomial. x beyond +-800 is clamped: the result is 0 or infinity there anyway. NaN stays NaN.
__device__ __forceinline__ double ard_exp(double x)
{
#pragma clang fp contract(off)
    x = x < -800.0 ? -800.0 : (x > 800.0 ? 800.0 : x);
    const double n = __builtin_rint(x * ard_const(1.44269504088896340736));
    double r = __builtin_fma(-n, ard_const(6.93147180369123816490e-01), x);
    r = __builtin_fma(-n, ard_const(1.90821492927058770002e-10), r);
    double p = ard_const(1.0 / 6227020800.0);
    p = __builtin_fma(p, r, ard_const(1.0 / 479001600.0));
    p = __builtin_fma(p, r, ard_const(1.0 / 39916800.0));
    p = __builtin_fma(p, r, ard_const(1.0 / 3628800.0));
    p = __builtin_fma(p, r, ard_const(1.0 / 362880.0));
    p = __builtin_fma(p, r, ard_const(1.0 / 40320.0));
    p = __builtin_fma(p, r, ard_const(1.0 / 5040.0));
    p = __builtin_fma(p, r, ard_const(1.0 / 720.0));
    p = __builtin_fma(p, r, ard_const(1.0 / 120.0));
    p = __builtin_fma(p, r, ard_const(1.0 / 24.0));
    p = __builtin_fma(p, r, ard_const(1.0 / 6.0));
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return __builtin_amdgcn_ldexp(p, (int)n);
}
// the same in fp32: degree 7 (remainder below 6e-9), n ln2_hi exact for |n| < 2^8, clamped beyond +-110
__device__ __forceinline__ float ard_exp(float x)
{
#pragma clang fp contract(off)
    x = x < -110.0f ? -110.0f : (x > 110.0f ? 110.0f : x);
    const float n = __builtin_rintf(x * 1.44269504f);
    float r = __builtin_fmaf(-n, 0.693145751953125f, x);
    r = __builtin_fmaf(-n, 1.42860677e-06f, r);
    float p = 1.0f / 5040.0f;
    p = __builtin_fmaf(p, r, 1.0f / 720.0f);
    p = __builtin_fmaf(p, r, 1.0f / 120.0f);
    p = __builtin_fmaf(p, r, 1.0f / 24.0f);
    p = __builtin_fmaf(p, r, 1.0f / 6.0f);
    p = __builtin_fmaf(p, r, 0.5f);
    p = __builtin_fmaf(p, r, 1.0f);
    p = __builtin_fmaf(p, r, 1.0f);
    return __builtin_amdgcn_ldexpf(p, (int)n);
}
__device__ __forceinline__ double ard_sqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float ard_sqrt(float v) { return sqrtf(v); }
// An element is finished HERE: without the pin hipcc sinks the evaluation of every tile's elements below the distance loops of all later
// tiles and keeps the squared distances of the whole triangle alive beside the accumulators (155 spilled registers in the fp64 6 x 6 form)
__device__ __forceinline__ void ard_pin(double &v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void ard_pin(float &v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ double ard_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float ard_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

//   SE:        phi = exp(-s / 2)                                    psi = phi
//   MATERN52:  phi = (1 + a + 5 s / 3) exp(-a),  a = sqrt(5 s)      psi = 5/3 (1 + a) exp(-a)
// One exponential either way: the kind (wave-uniform) selects its argument and the two factors in front (1 for SE: the product is exact).
template <class T>
__device__ __forceinline__ void ard_element(T s, int kind, T &phi, T &psi)
{
#pragma clang fp contract(off)
    T arg = (T)-0.5 * s, fphi = (T)1, fpsi = (T)1;
    if (kind == MATINV_COV_MATERN52) {
        const T a = ard_const((T)2.23606797749978969641) * ard_sqrt(s);  // sqrt 5
        const T b = (T)1 + a;
        arg = -a;
        const T c53 = ard_const((T)1.66666666666666666667);
        fphi = b + c53 * s;
        fpsi = c53 * b;
    }
    const T e = ard_exp(arg);
    phi = fphi * e;
    psi = fpsi * e;
}

// M[row][col] from s: sf2 phi, the noise on the diagonal
template <class T>
__device__ __forceinline__ T ard_m(T s, int kind, T sf2, T sn2, bool diag)
{
#pragma clang fp contract(off)
    T phi, psi;
    ard_element(s, kind, phi, psi);
    T v = sf2 * phi;
    if (diag) v = v + sn2;
    return v;
}

}  // namespace matinv
