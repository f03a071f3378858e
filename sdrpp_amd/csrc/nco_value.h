// The frequency translation's value, one expression for every kernel that forms it: the complex product,
// the two-level NCO table and x * phasor(i) (fir_rows.h and through it the channel chain and the spectrum
// launches; bank_kernels.h). The products are spelled with fmaf, so the bits do not depend on the
// translation unit's contraction; bank_kernels.h still includes this header under the channel chain's
// setting, as it does quad_value.h.
#pragma once
#include <hip/hip_runtime.h>

namespace sdrgpu {

// The contraction is spelled out: left to -ffp-contract=fast, a*b - c*d becomes fma(a, b, -cd) in one
// kernel and fma(-c, d, ab) in another (the SLP vectoriser's packed form picks the other product),
// and the spectrum launches' VFO stage 1 then differed from fir_rows_kernel's in the last bit
// (r4b: test_spectrum_vfo_fused). With explicit fmaf there is one rounding sequence everywhere.
__device__ __forceinline__ float2 cmulf(float2 a, float2 b) {
    return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}

// Two-level NCO table: phasor(i) = Phi[i >> 12] * Plo[i & 4095], with
// Plo[k] = exp(i w k) (fixed per configuration, fp64 -> float on the host) and
// Phi[j] = exp(i (theta0 + w 4096 j)) (per call, fp64 on the device). Two cached
// loads + one complex multiply per sample instead of an fp64 argument reduction
// and a sincos; error <= ~2 ulp of the phasor, no drift (theta0 is carried in
// double-double on the host).
constexpr int NCO_LO_BITS = 12;
constexpr int NCO_LO = 1 << NCO_LO_BITS;
__device__ __forceinline__ float2 nco_tab(const float2* __restrict__ phi, const float2* __restrict__ plo, long long i) {
    return cmulf(phi[i >> NCO_LO_BITS], plo[i & (NCO_LO - 1)]);
}

// channel::FrequencyXlator (frequency_xlator.h:43-50) at sample i of the call: xlator_kernel's expression
__device__ __forceinline__ float2 xlate_value(float2 x, const float2* __restrict__ phi, const float2* __restrict__ plo, long long i) {
    return cmulf(x, nco_tab(phi, plo, i));
}

}  // namespace sdrgpu
