// Bit-exact recurrences: include this header only from a translation unit built with
// -ffp-contract=off (loop_kernels.h says why).
//
// The per-sample steps of loop::AGC<T>, correction::DCBlocker<T>, filter::Deemphasis<T> and BroadcastFM's
// pilot PLL, and its stereo matrix, stated once for the single-stream kernels (loop_kernels.h: one workgroup
// per stream) and the stream banks (bank_audio_kernels.h, bank_wfm_kernels.h: one lane per stream). Every
// step is written in the reference's operation order.
#pragma once
#include "serial_chunks.h"   // amp_of / scale_of

namespace sdrgpu {

struct AgcParams {
    float setPoint, attack, invAttack, decay, invDecay, maxGain, maxOutputAmp;
    int enabled;
};

// loop::AGC<T>::process, the enabled branch (agc.h:96-123): the gain of a sample of amplitude inAmp.
// lookahead() is the largest amplitude from this sample to the end of the current call (agc.h:109-118); it
// is evaluated only where the clip test fires.
template <typename LookAhead>
__device__ __forceinline__ float agc_step(const AgcParams& p, float inAmp, float& amp, float& gain, LookAhead lookahead) {
    if (inAmp != 0.0f) {
        amp = (inAmp > amp) ? ((amp * p.invAttack) + (inAmp * p.attack))
                            : ((amp * p.invDecay) + (inAmp * p.decay));
        const float q = p.setPoint / amp;
        gain = (p.maxGain < q) ? p.maxGain : q;              // std::min<float>
    } else {
        gain = 1.0f;
    }
    if (inAmp * gain > p.maxOutputAmp) {                     // clip look-ahead
        amp = lookahead();
        const float q = p.setPoint / amp;
        gain = (p.maxGain < q) ? p.maxGain : q;
    }
    return gain;
}

// ... the disabled branch (agc.h:127-141): the fixed gain, limited to maxOutputAmp / inAmp
__device__ __forceinline__ float agc_fixed_step(const AgcParams& p, float inAmp, float gain) {
    return (inAmp * gain > p.maxOutputAmp) ? (p.maxOutputAmp / inAmp) : gain;
}

// DC blocker (dc_blocker.h:54-60): out = in - off; off += out * rate, per component
__device__ __forceinline__ float dcb_step(float x, float2& off, float rate) {
    const float o = x - off.x;
    off.x += o * rate;
    return o;
}
__device__ __forceinline__ float2 dcb_step(float2 v, float2& off, float rate) {
    const float ox = v.x - off.x, oy = v.y - off.y;
    off.x += ox * rate;
    off.y += oy * rate;
    return make_float2(ox, oy);
}

// filter::Deemphasis<T> (deephasis.h:57-77): out = alpha * in + (1 - alpha) * prev; beta = 1 - alpha
__device__ __forceinline__ float deemp_step(float alpha, float beta, float x, float& last) {
    const float y = (alpha * x) + (beta * last);
    last = y;
    return y;
}

// BroadcastFM's pilot PLL: loop/pll.h:64-70 + loop/phase_control_loop.h:59-66
struct PllParams {
    float alpha, beta, minPhase, maxPhase, phaseDelta, minFreq, maxFreq;
};
// One sample: th = the input's phase; returns the phase the VCO outputs for it (math::phasor(pcl.phase)
// BEFORE advance, pll.h:66-67), then advances (phase, freq).
__device__ __forceinline__ float pll_step(const PllParams& p, float th, float& phase, float& freq) {
    const float PI = 3.1415926535f;                             // FL_M_PI (math/constants.h:4)
    const float vco = phase;
    // (the two if / else-if chains of the reference as selects of the same values: a lane-per-stream wave
    // would otherwise branch on its lanes' union at every sample)
    const float d0 = th - phase;
    const float diff = d0 > PI ? d0 - 2.0f * PI : (d0 <= -PI ? d0 + 2.0f * PI : d0);   // math::normalizePhase
    const float f0 = freq + p.beta * diff;                      // PhaseControlLoop::advance
    freq = f0 > p.maxFreq ? p.maxFreq : (f0 < p.minFreq ? p.minFreq : f0);
    phase += freq + (p.alpha * diff);
    while (phase > p.maxPhase) phase -= p.phaseDelta;
    while (phase < p.minPhase) phase += p.phaseDelta;
    return vco;
}

// BroadcastFM stereo (demod/broadcast_fm.h:173-190) of one sample: d = the delayed MPX (Delay<float>, and the
// real part of Delay<complex_t>, whose input is RealToComplex of the MPX: its imaginary part is exactly 0),
// vcoPhase = the PLL's output phase. Conjugate(phasor), the two complex multiplies as the reference forms
// them (0 * x terms included, so they round identically), x2, then (l, r) = (L+R) + (L-R), (L+R) - (L-R).
__device__ __forceinline__ float2 stereo_matrix_value(float d, float vcoPhase) {
    const float vr = cosf(vcoPhase), vi = -sinf(vcoPhase);      // Conjugate(phasor)
    float ar = d, ai = 0.0f;
#pragma unroll
    for (int k = 0; k < 2; k++) {                               // Multiply<complex_t>, twice
        const float nr = (ar * vr) - (ai * vi);
        const float ni = (ai * vr) + (ar * vi);
        ar = nr;
        ai = ni;
    }
    const float lmr = ar * 2.0f;
    return make_float2(d + lmr, d - lmr);
}

}  // namespace sdrgpu
