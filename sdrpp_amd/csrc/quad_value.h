// The FM quadrature's value, one expression for every kernel that forms it (chain_kernels.h, fir_tile.h,
// fir_mfma.h, bank_kernels.h). Its products are left to the translation unit's contraction: the
// channel chain builds with the default (fast), and bank_kernels.h includes this header under the same
// setting so that its columns match.
#pragma once
#include <hip/hip_runtime.h>

namespace sdrgpu {

// atan2 of the FM quadrature (demod/quadrature.h:41-56: arg(y * conj(y[-1])) = complex_t::phase(), i.e.
// atan2f), for every kernel that forms it: OCML's atan2f, the device libm's correctly-signed,
// ~1-ulp counterpart of the reference's glibc atan2f (tests/test_ref_pinned.py pins it against the
// reference-code fixture). Round 3 measured a minimax polynomial with v_rcp_f32 instead (|error| <=
// 1.4 ulp(pi) absolute, far more ulps than that on small phase steps): C3 0.862 -> 0.850 ms, -1.3%
// (profiles/r3/c3_atan/). Not worth the parity concession: it stays an A/B build only
// (-DSDRGPU_POLY_ATAN2).
__device__ __forceinline__ float quad_atan2f(float y, float x) {
#ifndef SDRGPU_POLY_ATAN2
    return atan2f(y, x);
#else
    const float ax = fabsf(x), ay = fabsf(y);
    const bool swp = ay > ax;
    const float mn = swp ? ax : ay, mx = swp ? ay : ax;
    const float a = mn * __builtin_amdgcn_rcpf(mx == 0.0f ? 1.0f : mx);
    const float s = a * a;
    float p = 0.0028662257f;
    p = fmaf(p, s, -0.0161657367f);
    p = fmaf(p, s, 0.0429096138f);
    p = fmaf(p, s, -0.0752896400f);
    p = fmaf(p, s, 0.1065626393f);
    p = fmaf(p, s, -0.1420889944f);
    p = fmaf(p, s, 0.1999355085f);
    p = fmaf(p, s, -0.3333314528f);
    float r = fmaf(a * s, p, a);
    r = swp ? 1.57079632679489662f - r : r;
    r = signbit(x) ? 3.14159265358979324f - r : r;
    return copysignf(r, y);
#endif
}

// demod/quadrature.h:41-56: arg(y * conj(d)) / dev (one expression for every kernel using it)
__device__ __forceinline__ float quad_value(float2 y, float2 d, float invDev) {
    const float br = d.x, bi = -d.y;
    const float re = (y.x * br) - (y.y * bi);
    const float im = (y.y * br) + (y.x * bi);
    return quad_atan2f(im, re) * invDev;
}

}  // namespace sdrgpu
