// grad_px.h -- the per-pixel arithmetic of the gradient pass (myLSD.cpp:152-174), shared by K2 (k_grad.hip) and the fused front end
// (k_front.hip): both must take every pixel through the very same expressions.
#pragma once
#include "lsd_internal.h"
#include "devmath.h"

namespace lsdhip {

// fp32 angle with the two lowest mantissa bits replaced by the usedMap code (lsd_internal.h)
__device__ __forceinline__ uint32_t pack_pw(double d, uint32_t code) {
    return (__float_as_uint(__double2float_rn(d)) & ~3u) | code;
}

// The dense part of a pixel: gradient, magnitude, threshold code, and the angle where the gradient is zero.  A = G[y][x], B = G[y][x-1],
// C = G[y-1][x], D = G[y-1][x-1]; interior: x >= 1 && y >= 1 (Q3: row 0 / col 0 stay mag=0, deg=0, used=0).  heavy: the angle
// needs atan2 (grad_angle).
struct GradPx { double m, d, gradX, gradY; uint32_t u; bool heavy; };
__device__ __forceinline__ GradPx grad_pixel(double A, double B, double C, double D, bool interior, double gradThre) {
    GradPx p{0, 0, 0, 0, 0u, false};
    if (interior) {
        p.gradX = (B + D - A - C) / 2.0;                       // myLSD.cpp:161
        p.gradY = (C + D - A - B) / 2.0;                       // :162
        p.m = sqrt(p.gradX * p.gradX + p.gradY * p.gradY);     // :163 (pow(.,2) == x*x, Q12)
        if (p.m < gradThre) p.u = 1;                           // :165-166
        if (p.gradX == 0.0 && p.gradY == 0.0) {
            // atan2(+-0, -(+-0)) (:169) followed by the "pi -> 0" rule (:170-171): IEEE special cases
            if (signbit(-p.gradY)) p.d = signbit(p.gradX) ? -kPi : 0.0;
            else p.d = p.gradX;
        } else p.heavy = true;
    }
    return p;
}

// Level-line angle of a non-zero gradient (:169-171).  *tie is counted up where the angle lies within an ulp of atan2 of the rule's
// threshold: a decision another libm could take differently (lsd_last_sensitivity).
__device__ __forceinline__ double grad_angle(double gradX, double gradY, int32_t* tie) {
    double d;                                                  // :169 (first stage inline, second stage out of line: devmath.h)
    if (!crm::atan2_fast(gradX, -gradY, d)) d = atan2_g(gradX, -gradY);
    if (fabs(fabs(d - kPi) - 0.000001) <= 1e-14) atomicAdd(tie, 1);
    if (fabs(d - kPi) < 0.000001) d = 0;                       // :170-171
    return d;
}

// sin/cos(deg) for RegionGrower (:545-546)
__device__ __forceinline__ double2 grad_sincos(double d) {
    double sv, cv;
    if (!crm::sincos_fast(d, sv, cv)) sincos_g(d, sv, cv);
    return make_double2(sv, cv);
}

}  // namespace lsdhip
