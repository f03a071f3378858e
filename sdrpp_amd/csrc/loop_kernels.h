// Bit-exact recurrences: include this header only from a translation unit built with
// -ffp-contract=off (sdrpp_amd/build.py does that for loops.hip; HIP contracts a*b+c into an FMA
// by default, which rounds once where the reference rounds twice).
//
// Device code of loops.hip: the serial (data-dependent) loops of the demodulators and the
// elementwise kernels around them.
//   loop::AGC<T>                   loop/agc.h:88-147
//   correction::DCBlocker          correction/dc_blocker.h:54-60
//   noise_reduction::NoiseBlanker  noise_reduction/noise_blanker.h:38-57
//   filter::Deemphasis<T>          filter/deephasis.h:57-77
//   loop::PLL + the stereo matrix  demod/broadcast_fm.h:144-191, loop/pll.h:64-70
//
// The AGC, the DC blocker, the noise blanker, the de-emphasis and the PLL are first-order
// recurrences whose next state depends on the current sample (the AGC nonlinearly), so they run
// as ONE workgroup per stream: the block is walked in 1024-sample chunks; all 256 lanes stage the
// chunk (and, for the AGC, its amplitudes and the exact suffix maxima its clip look-ahead needs)
// in LDS, lane 0 runs the recurrence over the chunk from LDS, and all lanes write the chunk out
// (serial_chunks; the AGC, with its extra phases, is written out). Every step is written in the
// reference's order, and division / square root are IEEE (correctly rounded), so the GPU result is
// bit-identical to the reference arithmetic (oracle/sdr_oracle.c orc_agc / orc_dcb).
//
// The AGC's clip look-ahead scans amplitudes from sample i to the end of the CURRENT block
// (agc.h:109-118; O(n^2) worst case in the reference). The suffix maximum over the block is
// precomputed in parallel (max is exact), so the serial loop is O(n) and the result is the
// same value. State (average amplitude, gain; DC offset) stays on the device between calls.
#pragma once
#include "serial_chunks.h"   // LOOP_CHUNK / LOOP_NT, amp_of / scale_of, serial_chunks
#include "loop_steps.h"      // AgcParams, agc_step / agc_fixed_step, dcb_step, deemp_step, PllParams, pll_step,
                             // stereo_matrix_value (shared with the banks)

namespace sdrgpu {

// ---------------------------------------------------------------------- AGC
struct AgcState {
    float amp, gain;
};

// per-chunk amplitude maxima (exact), one workgroup per chunk
template <typename DT>
__global__ __launch_bounds__(LOOP_NT) void chunk_max_kernel(const DT* __restrict__ in, int count, float* __restrict__ cm) {
    __shared__ float red[LOOP_NT];
    const int c = blockIdx.x;
    float m = 0.0f;
    for (int i = c * LOOP_CHUNK + threadIdx.x; i < min(count, (c + 1) * LOOP_CHUNK); i += LOOP_NT) m = fmaxf(m, amp_of(in[i]));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = LOOP_NT / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) cm[c] = red[0];
}

// One workgroup: the whole block, chunk by chunk. `cm` holds the chunk maxima on entry.
template <typename DT>
__global__ __launch_bounds__(LOOP_NT) void agc_kernel(const DT* __restrict__ in, DT* __restrict__ out, int count,
                                                      AgcParams p, AgcState* __restrict__ st, float* __restrict__ cm,
                                                      const float* __restrict__ setGain) {
    __shared__ DT X[LOOP_CHUNK];
    __shared__ float A[LOOP_CHUNK], S[LOOP_CHUNK], G[LOOP_CHUNK];
    const int t = threadIdx.x;
    const int nchunks = (count + LOOP_CHUNK - 1) / LOOP_CHUNK;
    if (t == 0) {   // cm[c] <- max over chunks > c (the look-ahead beyond chunk c)
        float run = 0.0f;
        for (int c = nchunks - 1; c >= 0; c--) {
            const float v = cm[c];
            cm[c] = run;
            run = fmaxf(run, v);
        }
    }
    __syncthreads();
    float amp = st->amp, gain = st->gain;
    if (setGain) gain = *setGain;                          // AGC::setGain latched at this call
    for (int c = 0; c < nchunks; c++) {
        const int i0 = c * LOOP_CHUNK;
        const int n = min(LOOP_CHUNK, count - i0);
        for (int i = t; i < LOOP_CHUNK; i += LOOP_NT) {
            if (i < n) {
                const DT v = in[i0 + i];
                X[i] = v;
                A[i] = amp_of(v);
            } else {
                A[i] = 0.0f;
            }
        }
        __syncthreads();
        if (p.enabled) {
            // S[i] = max(A[i..n-1], beyond): Hillis-Steele suffix max, exact
            for (int i = t; i < LOOP_CHUNK; i += LOOP_NT) S[i] = (i == n - 1) ? fmaxf(A[i], cm[c]) : A[i];
            __syncthreads();
            for (int d = 1; d < LOOP_CHUNK; d <<= 1) {
                float v[LOOP_CHUNK / LOOP_NT];
#pragma unroll
                for (int k = 0; k < LOOP_CHUNK / LOOP_NT; k++) {
                    const int i = t + k * LOOP_NT;
                    v[k] = (i + d < n) ? fmaxf(S[i], S[i + d]) : S[i];
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < LOOP_CHUNK / LOOP_NT; k++) S[t + k * LOOP_NT] = v[k];
                __syncthreads();
            }
        }
        if (t == 0) {
            if (p.enabled) {
                for (int i = 0; i < n; i++) G[i] = agc_step(p, A[i], amp, gain, [&] { return S[i]; });
            } else {
                for (int i = 0; i < n; i++) G[i] = agc_fixed_step(p, A[i], gain);
            }
        }
        __syncthreads();
        for (int i = t; i < n; i += LOOP_NT) out[i0 + i] = scale_of(X[i], G[i]);
        __syncthreads();
    }
    if (t == 0) {
        st->amp = amp;
        st->gain = gain;
    }
}

// ------------------------------------------------------- elementwise maps
// volk_32fc_magnitude_32f (AM) / ComplexToReal (SSB) / MonoToStereo / convert::RealToComplex /
// complex_t::phase() (types.h:57)
__global__ void magnitude_kernel(const float2* __restrict__ in, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = amp_of(in[i]);
}
__global__ void real_part_kernel(const float2* __restrict__ in, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i].x;
}
__global__ void mono_to_stereo_kernel(const float* __restrict__ in, float2* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = make_float2(in[i], in[i]);
}
__global__ void real_to_complex_kernel(const float* __restrict__ in, float2* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = make_float2(in[i], 0.0f);
}
__global__ void phase_kernel(const float2* __restrict__ in, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = atan2f(in[i].y, in[i].x);
}

// BroadcastFM stereo (demod/broadcast_fm.h:144-191): the delays, then stereo_matrix_value (loop_steps.h),
// written (l, r) as a float2 pair for the audio FIR.
__global__ void stereo_matrix_kernel(const float* __restrict__ mpx, const float* __restrict__ hist, int delay,
                                     const float* __restrict__ vcoPhase, float2* __restrict__ lr, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float d = i < delay ? hist[i] : mpx[i - delay];       // Delay<float> / Delay<complex_t>.re
    lr[i] = stereo_matrix_value(d, vcoPhase[i]);
}


// ------------------------------------------------- the serial_chunks blocks
// DC blocker (dc_blocker.h:54-60): out = in - off; off += out * rate, per component
template <typename DT>
__global__ __launch_bounds__(LOOP_NT) void dcb_kernel(const DT* __restrict__ in, DT* __restrict__ out, int count,
                                                      float rate, float2* __restrict__ st) {
    __shared__ DT X[LOOP_CHUNK];
    float2 off = *st;
    serial_chunks(
        count, [&](int i0, int i) { X[i] = in[i0 + i]; },
        [&](int i) { X[i] = dcb_step(X[i], off, rate); },
        [&](int i0, int i) { out[i0 + i] = X[i]; });
    if (threadIdx.x == 0) *st = off;
}

// noise_reduction::NoiseBlanker (noise_reduction/noise_blanker.h:38-57): the running amplitude
// follows every non-zero sample; a sample more than `level` times above it is scaled back to it
struct NbParams {
    float rate, invRate, level;
};
__global__ __launch_bounds__(LOOP_NT) void noise_blanker_kernel(const float2* __restrict__ in, float2* __restrict__ out, int count,
                                                               NbParams p, float* __restrict__ st) {
    __shared__ float2 X[LOOP_CHUNK];
    __shared__ float A[LOOP_CHUNK], G[LOOP_CHUNK];
    float amp = *st;
    serial_chunks(
        count,
        [&](int i0, int i) {
            const float2 v = in[i0 + i];
            X[i] = v;
            A[i] = amp_of(v);
        },
        [&](int i) {
            const float inAmp = A[i];
            float gain = 1.0f;
            if (inAmp != 0.0f) {
                amp = (amp * p.invRate) + (inAmp * p.rate);
                const float excess = inAmp / amp;
                if (excess > p.level) gain = 1.0f / excess;
            }
            G[i] = gain;
        },
        [&](int i0, int i) { out[i0 + i] = scale_of(X[i], G[i]); });
    if (threadIdx.x == 0) *st = amp;
}

// filter::Deemphasis<T> (filter/deephasis.h:57-77): out = alpha * in + (1 - alpha) * prev,
// per channel (float: 1, stereo_t: 2); prev carried on the device
template <int C>
__global__ __launch_bounds__(LOOP_NT) void deemp_kernel(const float* __restrict__ in, float* __restrict__ out, int count,
                                                        float alpha, float2* __restrict__ st) {
    __shared__ float X[LOOP_CHUNK * C];
    float last[2] = {st->x, st->y};
    const float beta = 1 - alpha;                               // (1 - alpha): int - float -> float
    serial_chunks<C>(
        count, [&](int i0, int e) { X[e] = in[(size_t)i0 * C + e]; },
        [&](int i) {
#pragma unroll
            for (int c = 0; c < C; c++) X[i * C + c] = deemp_step(alpha, beta, X[i * C + c], last[c]);
        },
        [&](int i0, int e) { out[(size_t)i0 * C + e] = X[e]; });
    if (threadIdx.x == 0) *st = make_float2(last[0], last[1]);
}

// BroadcastFM's pilot PLL (pll_step, loop_steps.h), one workgroup: in place, th[i] = input phase -> the
// phase the VCO outputs for sample i (math::phasor(pcl.phase) BEFORE advance). State (phase, freq) on device.
__global__ __launch_bounds__(LOOP_NT) void pll_kernel(float* __restrict__ th, int count, PllParams p, float2* __restrict__ st) {
    __shared__ float T[LOOP_CHUNK];
    float phase = st->x, freq = st->y;
    serial_chunks(
        count, [&](int i0, int i) { T[i] = th[i0 + i]; },
        [&](int i) { T[i] = pll_step(p, T[i], phase, freq); },
        [&](int i0, int i) { th[i0 + i] = T[i]; });
    if (threadIdx.x == 0) *st = make_float2(phase, freq);
}

}  // namespace sdrgpu
