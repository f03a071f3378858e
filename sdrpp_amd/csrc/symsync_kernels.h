// Bit-exact recurrences: include this header only from a translation unit built with
// -ffp-contract=off (sdrpp_amd/build.py does that for symsync.hip; HIP contracts a*b+c into an FMA
// by default, which rounds once where the reference rounds twice).
//
// Device code of symsync.hip: symbol recovery.
//   loop::FastAGC<T>                 loop/fast_agc.h:60-79
//   loop::Costas<ORDER>              loop/costas.h:17-45, loop/phase_control_loop.h:58-85
//   loop::MeteorCostas               decoder_modules/meteor_demodulator/src/meteor_costas.h:24-56, and the
//                                    OQPSK stagger of demod::Meteor (meteor_demod.h:155-164)
//   loop::PLL, CarrierTrackingPLL    loop/pll.h:64-70, loop/carrier_tracking_pll.h:14-20
//   clock_recovery::MM<T>            clock_recovery/mm.h:100-156
//   digital::BinarySlicer            digital/binary_slicer.h:12-18
//   digital::DifferentialDecoder     digital/differential_decoder.h:41-47
//
// The three loops are data-dependent recurrences: one workgroup of LOOP_NT lanes per stream walks the
// call in LOOP_CHUNK-sample chunks staged in LDS, lane 0 runs the recurrence in the reference's
// operation order, all lanes store the results (serial_chunks.h). State lives on the device between
// calls and is written back by lane 0. Nothing here uses atomics. The per-sample step of each loop is a
// __forceinline__ function (fast_agc_step, costas_step, meteor_costas_step, mm_step; pll_step of
// loop_steps.h) that the lane-per-stream kernels of bank_kernels.h call too: a recurrence is stated once.
#pragma once
#include "serial_chunks.h"
#include "loop_steps.h"   // PllParams, pll_step

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
// one sample of a loop that derotates by its phase (costas.h:17-24, meteor_costas.h:24-30 over
// phase_control_loop.h:58-85): the derotated sample out, the loop moved on by error(re, im) of that sample
template <typename Err>
__device__ __forceinline__ float2 derotate_step(const PclParams& p, float2 v, float& phase, float& freq, Err error) {
    const float PI = 3.1415926535f;                            // FL_M_PI (math/constants.h:4)
    const float minPhase = -PI, maxPhase = PI, phaseDelta = maxPhase - minPhase;
    const float vr = cosf(-phase), vi = sinf(-phase);           // math::phasor(-pcl.phase)
    const float re = (v.x * vr) - (v.y * vi);                   // complex_t::operator* (types.h:23)
    const float im = (v.y * vr) + (v.x * vi);
    pcl_advance(p, error(re, im), phase, freq);
    while (phase > maxPhase) phase -= phaseDelta;               // clampPhase (:82-85)
    while (phase < minPhase) phase += phaseDelta;
    return make_float2(re, im);
}
template <int ORDER>
__device__ __forceinline__ float2 costas_step(const PclParams& p, float2 v, float& phase, float& freq) {
    return derotate_step(p, v, phase, freq, [](float re, float im) { return costas_error<ORDER>(re, im); });
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

// ------------------------------------------------------------- MeteorCostas
// math::normalizePhase (math/normalize_phase.h:6-10), the if / else-if as selects of the same values
// (pll_step, loop_steps.h, says why)
__device__ __forceinline__ float normalize_phase(float d) {
    const float PI = 3.1415926535f;
    return d > PI ? d - 2.0f * PI : (d <= -PI ? d + 2.0f * PI : d);
}
// meteor_costas.h:33-56. `broken` is the launch's, not the sample's: the branch is uniform. Without it the
// error is Costas<4>'s to the letter (:53, :55). With it: the distance of the sample's phase to the
// nearest of four unevenly spaced constellation phases, scaled by its amplitude.
__device__ __forceinline__ float meteor_costas_error(float re, float im, int broken) {
    if (!broken) return costas_error<4>(re, im);
    const float PHASE1 = (float)0.47439988279190737, PHASE2 = (float)2.1777839908413044;   // :36-39, const float = double
    const float PHASE3 = (float)3.8682349942715186, PHASE4 = (float)-0.29067248091319986;
    const float phase = atan2f(im, re);                         // complex_t::phase() (types.h:57-59)
    const float dp1 = normalize_phase(phase - PHASE1), dp2 = normalize_phase(phase - PHASE2);
    const float dp3 = normalize_phase(phase - PHASE3), dp4 = normalize_phase(phase - PHASE4);
    float lowest = dp1;                                         // :46-49, strict comparisons in this order
    lowest = fabsf(dp2) < fabsf(lowest) ? dp2 : lowest;
    lowest = fabsf(dp3) < fabsf(lowest) ? dp3 : lowest;
    lowest = fabsf(dp4) < fabsf(lowest) ? dp4 : lowest;
    const float err = lowest * amp_of(make_float2(re, im));    // :50, complex_t::amplitude() (types.h:79)
    return (err < -1.0f) ? -1.0f : ((1.0f < err) ? 1.0f : err);   // std::clamp<float>
}
__device__ __forceinline__ float2 meteor_costas_step(const PclParams& p, int broken, float2 v, float& phase, float& freq) {
    return derotate_step(p, v, phase, freq, [broken](float re, float im) { return meteor_costas_error(re, im, broken); });
}
// demod::Meteor's OQPSK stagger of one sample (meteor_demod.h:157-161): the Q arm one sample late
__device__ __forceinline__ float2 oqpsk_stagger(float2 o, float& lastI) {
    const float tmp = o.y;
    o.y = lastI;
    lastI = tmp;
    return o;
}
struct MeteorCostasParams {
    CostasParams c;
    int broken;   // setBrokenModulation (:18-22): a parameter of the call, the loop state is kept
    int oqpsk;    // demod::Meteor's stagger on the loop's output (off for a MeteorCostas of its own)
};
// state: (phase, freq); lastI apart from it (Meteor::reset, meteor_demod.h:139-148, does not touch it), read
// and written only while the stagger is on. The stagger is data movement on the value lane 0 has in hand.
static __global__ __launch_bounds__(LOOP_NT) void meteor_costas_kernel(const float2* __restrict__ in, float2* __restrict__ out,
                                                                       int count, MeteorCostasParams p,
                                                                       float2* __restrict__ st, float* __restrict__ lastIp) {
    __shared__ float2 X[LOOP_CHUNK];
    float phase = st->x, freq = st->y;
    float lastI = p.oqpsk ? *lastIp : 0.0f;
    if (p.c.clampNow) pcl_clamp_freq(p.c.pcl, freq);
    serial_chunks(
        count, [&](int i0, int i) { X[i] = in[i0 + i]; },
        [&](int i) {
            const float2 o = meteor_costas_step(p.c.pcl, p.broken, X[i], phase, freq);
            X[i] = p.oqpsk ? oqpsk_stagger(o, lastI) : o;
        },
        [&](int i0, int i) { out[i0 + i] = X[i]; });
    if (threadIdx.x == 0) {
        *st = make_float2(phase, freq);
        if (p.oqpsk) *lastIp = lastI;
    }
}

// ------------------------------------------------- PLL, CarrierTrackingPLL
// Both run pll_step (loop_steps.h) on the phase of the INPUT sample (pll.h:67, carrier_tracking_pll.h:17) and
// differ in what they emit for the VCO phase taken before the advance: its phasor (pll.h:66), or the input
// derotated by it (carrier_tracking_pll.h:16).
template <bool DEROTATE>
__device__ __forceinline__ float2 pll_output(float2 v, float vco) {
    if constexpr (!DEROTATE) {
        return make_float2(cosf(vco), sinf(vco));               // math::phasor(pcl.phase)
    } else {
        const float vr = cosf(-vco), vi = sinf(-vco);           // math::phasor(-pcl.phase)
        return make_float2((v.x * vr) - (v.y * vi), (v.y * vr) + (v.x * vi));   // complex_t::operator* (types.h:23)
    }
}
// Only pll_step is serial: all lanes take atan2f of the chunk's inputs, lane 0 turns the input phases into
// VCO phases, all lanes form the outputs. state: (phase, freq)
template <bool DEROTATE>
__global__ __launch_bounds__(LOOP_NT) void carrier_pll_kernel(const float2* __restrict__ in, float2* __restrict__ out, int count,
                                                              PllParams p, int clampNow, float2* __restrict__ st) {
    __shared__ float2 X[LOOP_CHUNK];
    __shared__ float T[LOOP_CHUNK];
    float phase = st->x, freq = st->y;
    if (clampNow) freq = freq > p.maxFreq ? p.maxFreq : (freq < p.minFreq ? p.minFreq : freq);   // setFreqLimits (:51-56)
    serial_chunks(
        count,
        [&](int i0, int i) {
            const float2 v = in[i0 + i];
            X[i] = v;
            T[i] = atan2f(v.y, v.x);                            // complex_t::phase() (types.h:57-59)
        },
        [&](int i) { T[i] = pll_step(p, T[i], phase, freq); },
        [&](int i0, int i) { out[i0 + i] = pll_output<DEROTATE>(X[i], T[i]); });
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

// ------------------------------------------------- FIR in the reference's order
// The stream banks' FIR (bank_kernels.h has the layout: element m of stream k at x[m S + k], so the S streams are
// one flat stream of S-vectors and the sample before element i is element i - S; one thread per element i = m S + k,
// coalesced over k). demod::Meteor's single-stream chain runs it with S = 1: its RRC then sums exactly as the
// reference's VOLK generic kernel does, and a BankMeteor column is the single-stream chain bit for bit.
// filter/fir.h:60-80 per stream: out[m S + k] = sum_j buf_k[m + j] taps[j] over [hist (T - 1 rows) || in],
// ascending taps, fp32, unfused (this translation unit does not contract): the sum does not depend on
// how the rows are cut into calls. n = frames * S elements, HS = (T - 1) * S history elements. The
// history carry is carry_history (blocks.h) over the flat stream.
template <typename DT>
__global__ void bank_fir_kernel(const DT* __restrict__ in, DT* __restrict__ out, int n, int S, int HS,
                                const float* __restrict__ taps, int T, const DT* __restrict__ hist) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // (the grid's last block may pass INT_MAX)
    if (i >= n) return;
    DT acc{};
    for (int j = 0; j < T; j++) {
        const long long b = i + (long long)j * S;   // element of [hist || in]
        const DT x = b < HS ? hist[b] : in[b - HS];
        const float t = taps[j];
        if constexpr (sizeof(DT) == 4) {
            acc += x * t;
        } else {
            acc.x += x.x * t;
            acc.y += x.y * t;
        }
    }
    out[i] = acc;
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
