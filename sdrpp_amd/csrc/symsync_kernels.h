// Bit-exact recurrences: include this header only from a translation unit built with
// -ffp-contract=off (sdrpp_amd/build.py does that for symsync.hip; HIP contracts a*b+c into an FMA
// by default, which rounds once where the reference rounds twice).
//
// Device code of symsync.hip: symbol recovery.
//   loop::FastAGC<T>                 loop/fast_agc.h:60-79
//   loop::Costas<ORDER>              loop/costas.h:17-45, loop/phase_control_loop.h:58-85
//   clock_recovery::MM<T>            clock_recovery/mm.h:100-156
//   digital::BinarySlicer            digital/binary_slicer.h:12-18
//   digital::DifferentialDecoder     digital/differential_decoder.h:41-47
//
// The three loops are data-dependent recurrences: one workgroup of LOOP_NT lanes per stream walks the
// call in LOOP_CHUNK-sample chunks staged in LDS, lane 0 runs the recurrence in the reference's
// operation order, all lanes store the results (serial_chunks.h). State lives on the device between
// calls and is written back by lane 0. Nothing here uses atomics. The per-sample step of each loop is a
// __forceinline__ function (fast_agc_step, costas_step, mm_step) that the lane-per-stream kernels of
// bank_kernels.h call too: a recurrence is stated once.
#pragma once
#include "serial_chunks.h"

namespace sdrgpu {

// math::step (math/step.h:5-17)
__device__ __forceinline__ float step_of(float x) { return (x > 0.0f) ? 1.0f : -1.0f; }

// PhaseControlLoop<float>::advance (phase_control_loop.h:58-66) without the phase clamp
struct PclParams {
    float alpha, beta, minFreq, maxFreq;
};
__device__ __forceinline__ void pcl_clamp_freq(const PclParams& p, float& freq) {   // :77-80
    if (freq > p.maxFreq) freq = p.maxFreq;
    else if (freq < p.minFreq) freq = p.minFreq;
}
__device__ __forceinline__ void pcl_advance(const PclParams& p, float error, float& phase, float& freq) {
    freq += p.beta * error;
    pcl_clamp_freq(p, freq);
    phase += freq + (p.alpha * error);
}

// ------------------------------------------------------------------ FastAGC
struct FastAgcParams {
    float setPoint, maxGain, rate;
    float setGain;   // FastAGC::setGain latched at this call ...
    int hasGain;     // ... when non-zero
};
// one sample (fast_agc.h:66-76): the scaled sample out, the gain moved on
template <typename DT>
__device__ __forceinline__ DT fast_agc_step(const FastAgcParams& p, DT x, float& gain) {
    const DT o = scale_of(x, gain);
    const float amp = amp_of(o);
    gain += (p.setPoint - amp) * p.rate;
    if (gain > p.maxGain) gain = p.maxGain;
    return o;
}
template <typename DT>
__global__ __launch_bounds__(LOOP_NT) void fast_agc_kernel(const DT* __restrict__ in, DT* __restrict__ out, int count,
                                                           FastAgcParams p, float* __restrict__ st) {
    __shared__ DT X[LOOP_CHUNK];
    float gain = p.hasGain ? p.setGain : *st;
    serial_chunks(
        count, [&](int i0, int i) { X[i] = in[i0 + i]; },
        [&](int i) { X[i] = fast_agc_step(p, X[i], gain); },
        [&](int i0, int i) { out[i0 + i] = X[i]; });
    if (threadIdx.x == 0) *st = gain;
}

// ------------------------------------------------------------------- Costas
struct CostasParams {
    PclParams pcl;
    int clampNow;   // PLL::setFrequencyLimits since the last call: clampFreq before the first sample (:51-56)
};
template <int ORDER>
__device__ __forceinline__ float costas_error(float re, float im) {   // costas.h:26-45
    float err;
    if constexpr (ORDER == 2) {
        err = re * im;
    } else if constexpr (ORDER == 4) {
        err = (step_of(re) * im) - (step_of(im) * re);
    } else {
        const float K = sqrtf(2.0f) - 1.0f;   // (float)((double)sqrtf(2.0) - 1.0): the difference is exact
        if (fabsf(re) >= fabsf(im)) err = (step_of(re) * im) - ((step_of(im) * re) * K);
        else err = ((step_of(re) * im) * K) - (step_of(im) * re);
    }
    return (err < -1.0f) ? -1.0f : ((1.0f < err) ? 1.0f : err);   // std::clamp<float>
}
// one sample (costas.h:17-24, phase_control_loop.h:58-85): the derotated sample out, the loop moved on
template <int ORDER>
__device__ __forceinline__ float2 costas_step(const PclParams& p, float2 v, float& phase, float& freq) {
    const float PI = 3.1415926535f;                            // FL_M_PI (math/constants.h:4)
    const float minPhase = -PI, maxPhase = PI, phaseDelta = maxPhase - minPhase;
    const float vr = cosf(-phase), vi = sinf(-phase);           // math::phasor(-pcl.phase)
    const float re = (v.x * vr) - (v.y * vi);                   // complex_t::operator* (types.h:23)
    const float im = (v.y * vr) + (v.x * vi);
    pcl_advance(p, costas_error<ORDER>(re, im), phase, freq);
    while (phase > maxPhase) phase -= phaseDelta;               // clampPhase (:82-85)
    while (phase < minPhase) phase += phaseDelta;
    return make_float2(re, im);
}
// state: (phase, freq)
template <int ORDER>
__global__ __launch_bounds__(LOOP_NT) void costas_kernel(const float2* __restrict__ in, float2* __restrict__ out, int count,
                                                         CostasParams p, float2* __restrict__ st) {
    __shared__ float2 X[LOOP_CHUNK];
    float phase = st->x, freq = st->y;
    if (p.clampNow) pcl_clamp_freq(p.pcl, freq);
    serial_chunks(
        count, [&](int i0, int i) { X[i] = in[i0 + i]; },
        [&](int i) { X[i] = costas_step<ORDER>(p.pcl, X[i], phase, freq); },
        [&](int i0, int i) { out[i0 + i] = X[i]; });
    if (threadIdx.x == 0) *st = make_float2(phase, freq);
}

// ----------------------------------------------------------------------- MM
constexpr int MM_MAX_TAPS = SDRGPU_MM_MAX_TAPS;
constexpr int MM_LDS_BANK = 4096;   // a bank of up to this many floats (the default 128 x 8: 1024) is staged in LDS

enum class MmEpilogue {
    Soft,       // the interpolated symbols (T)
    DiffBits,   // BinarySlicer -> DifferentialDecoder bits (uint8) out, the soft symbols into `soft` (float only)
};
struct MmState {
    int offset;
    float phase, freq;
    float lastOut;                       // MM<float>
    float2 p0, p1, p2, c0, c1, c2;      // MM<complex_t>: _p_0T .. _c_2T
    int lastSym;                         // DiffBits: the decoder's `last`
    int outCount;                        // outputs of the last call (the host reads it)
};
struct MmParams {
    PclParams pcl;      // alpha = muGain, beta = omegaGain, the omega limits
    float omega;
    int P, T;           // interpolator bank: P phases of T taps
    int inStride;       // floats between consecutive input samples (2: the real part of a complex_t stream)
    int modulus;        // DiffBits
    int setOmega;       // setOmega since the last call: offset = 0, phase = 0, freq = omega, clampFreq (mm.h:40-50)
    int clampNow;       // setOmegaRelLimit since the last call: clampFreq (mm.h:66-71)
};

template <typename DT>
__device__ __forceinline__ DT mm_load(const DT* in, size_t i, int stride) {
    if constexpr (sizeof(DT) == 4) return in[i * stride];
    else return in[i];
}

// One output (mm.h:109-147) at the loop state s: the interpolated symbol out; the error, the loop and the
// offset moved on. x(k): sample k of the work buffer from s.offset; b(ph, k): tap k of interpolator phase ph.
template <typename DT, typename XF, typename BF>
__device__ __forceinline__ DT mm_step(const MmParams& p, MmState& s, XF x, BF b) {
    // mm.h:111: clamp<int>(floorf(phase * P), 0, P - 1)
    int ph = (int)floorf(s.phase * (float)p.P);
    ph = ph < 0 ? 0 : (ph > p.P - 1 ? p.P - 1 : ph);
    DT o;
    float error;
    if constexpr (sizeof(DT) == 4) {
        float acc = 0.0f;                    // volk_32f_x2_dot_prod_32f_generic
        for (int k = 0; k < p.T; k++) acc += x(k) * b(ph, k);
        o = acc;
        error = (step_of(s.lastOut) * acc) - (s.lastOut * step_of(acc));   // :122-123
        s.lastOut = acc;
    } else {
        float ar = 0.0f, ai = 0.0f;          // volk_32fc_32f_dot_prod_32fc_generic
        for (int k = 0; k < p.T; k++) {
            const DT v = x(k);
            const float t = b(ph, k);
            ar += v.x * t;
            ai += v.y * t;
        }
        o = make_float2(ar, ai);
        s.p2 = s.p1; s.p1 = s.p0; s.c2 = s.c1; s.c1 = s.c0;            // :127-134
        s.p0 = make_float2(ar, ai);
        s.c0 = make_float2(step_of(ar), step_of(ai));
        // :137 (((p0 - p2) * c1.conj()) - ((c0 - c2) * p1.conj())).re
        const float dr = s.p0.x - s.p2.x, di = s.p0.y - s.p2.y;
        const float er = s.c0.x - s.c2.x, ei = s.c0.y - s.c2.y;
        const float a = (dr * s.c1.x) - (di * (-s.c1.y));
        const float c = (er * s.p1.x) - (ei * (-s.p1.y));
        error = a - c;
    }
    if (error > 1.0f) error = 1.0f;          // :141-142
    if (error < -1.0f) error = -1.0f;
    pcl_advance(p.pcl, error, s.phase, s.freq);
    const float delta = floorf(s.phase);
    s.offset = (int)((float)s.offset + delta);   // int += float
    s.phase -= delta;
    return o;
}

// One workgroup. The work buffer of mm.h:102 is [hist (T - 1 samples) || in (count samples)]; chunk c
// stages its elements [i0, i0 + n + T - 1) in LDS, lane 0 makes the outputs whose offset falls in
// [i0, i0 + n) and appends them to LDS, all lanes flush them. Every output advances offset by at least
// 1 (the host checks the parameters), so a chunk makes at most n outputs; the loop also stops there,
// which bounds it where a NaN has made the loop state meaningless.
template <typename DT, MmEpilogue EPI>
__global__ __launch_bounds__(LOOP_NT) void mm_kernel(const DT* __restrict__ in, int count, void* __restrict__ outv,
                                                     float* __restrict__ soft, MmParams p, const float* __restrict__ bank,
                                                     DT* __restrict__ hist, MmState* __restrict__ stp) {
    __shared__ DT W[LOOP_CHUNK + MM_MAX_TAPS - 1];
    __shared__ DT O[LOOP_CHUNK];
    __shared__ float BL[MM_LDS_BANK];
    __shared__ int nOut;
    const int t = threadIdx.x;
    const int T = p.T, H = p.T - 1;
    MmState s = *stp;
    if (p.setOmega) {
        s.offset = 0;
        s.phase = 0.0f;
        s.freq = p.omega;
    }
    if (p.setOmega || p.clampNow) pcl_clamp_freq(p.pcl, s.freq);
    const bool bankLds = p.P * T <= MM_LDS_BANK;
    if (bankLds)
        for (int i = t; i < p.P * T; i += LOOP_NT) BL[i] = bank[i];
    const float* B = bankLds ? BL : bank;
    int lastSym = s.lastSym;
    int outBase = 0;
    for (int i0 = 0; i0 < count; i0 += LOOP_CHUNK) {
        const int n = min(LOOP_CHUNK, count - i0);
        for (int e = t; e < n + H; e += LOOP_NT) {
            const int w = i0 + e;                        // index into the work buffer
            W[e] = w < H ? hist[w] : mm_load(in, (size_t)(w - H), p.inStride);
        }
        __syncthreads();
        if (t == 0) {
            int no = 0;
            while (s.offset >= i0 && s.offset < i0 + n && no < n) {
                const DT* x = &W[s.offset - i0];
                O[no++] = mm_step<DT>(p, s, [&](int k) { return x[k]; }, [&](int ph, int k) { return B[ph * T + k]; });
            }
            nOut = no;
        }
        __syncthreads();
        const int no = nOut;
        for (int j = t; j < no; j += LOOP_NT) {
            if constexpr (EPI == MmEpilogue::Soft) {
                reinterpret_cast<DT*>(outv)[outBase + j] = O[j];
            } else {
                static_assert(sizeof(DT) == 4, "the bit epilogue slices float symbols");
                const int cur = O[j] > 0.0f;             // binary_slicer.h:15
                const int prev = j > 0 ? (int)(O[j - 1] > 0.0f) : lastSym;
                reinterpret_cast<uint8_t*>(outv)[outBase + j] = (uint8_t)((cur - prev + p.modulus) % p.modulus);   // differential_decoder.h:43
                soft[outBase + j] = O[j];
            }
        }
        if constexpr (EPI == MmEpilogue::DiffBits) {
            if (no > 0) lastSym = O[no - 1] > 0.0f;
        }
        outBase += no;
        __syncthreads();
    }
    // :150-153 offset -= count; the last T - 1 work-buffer samples become the history (one workgroup:
    // every lane holds its sample before any lane writes)
    DT keep{};
    if (t < H) {
        const int w = count + t;
        keep = w < H ? hist[w] : mm_load(in, (size_t)(w - H), p.inStride);
    }
    __syncthreads();
    if (t < H) hist[t] = keep;
    if (t == 0) {
        s.offset -= count;
        s.lastSym = lastSym;
        s.outCount = outBase;
        *stp = s;
    }
}

// --------------------------------------------------- slicer, differential decoder
// (static: bank_kernels.h includes this header from a second translation unit)
static __global__ void slicer_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] > 0.0f;
}
// last[0]: the symbol before in[0]; last[1] <- in[n - 1] (the host swaps the two per call)
static __global__ void diff_decode_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int n, int modulus,
                                   const int* __restrict__ last, int* __restrict__ next) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int cur = in[i];
    const int prev = i > 0 ? (int)in[i - 1] : *last;
    out[i] = (uint8_t)((cur - prev + modulus) % modulus);
    if (i == n - 1) *next = cur;
}

}  // namespace sdrgpu
