// Bit-exact recurrences: include this header only from a translation unit built with
// -ffp-contract=off (loop_kernels.h says why).
//
// The per-sample steps of loop::AGC<T>, correction::DCBlocker<T> and filter::Deemphasis<T>, stated once
// for the single-stream kernels (loop_kernels.h: one workgroup per stream) and the stream banks
// (bank_audio_kernels.h: one lane per stream). Every step is written in the reference's operation order.
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

}  // namespace sdrgpu
