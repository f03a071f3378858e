// Bit-exact recurrences: include this header only from a translation unit built with
// -ffp-contract=off (sdrpp_amd/build.py does that for bank.hip; loop_kernels.h says why).
//
// Device code of bank.hip, the analogue receiver banks (the layout and the lane-per-stream walk are in
// bank_kernels.h):
//   loop::AGC<T>, correction::DCBlocker<T>,
//   filter::Deemphasis<float | stereo_t>       one lane per stream, on the steps of loop_steps.h
//   noise_reduction::Squelch                   column sums in a fixed order, a lane-per-stream decision, a gate
//   volk_32fc_magnitude_32f                    one thread per element of the flat frames * S stream
//
// The AGC's clip look-ahead is the largest |x| over rows [i, frames) of the current call, per stream
// (agc.h:109-118). A pre-pass (bank_tile_max_kernel, a tiles x waves grid straight from global memory,
// no LDS) leaves the maximum of every BANK_F-row tile of every stream in tm[t * S + k]; the walk's lane
// first turns its own column of tm into the exclusive suffix (the maximum over all LATER tiles), and where
// the clip test fires at row r of tile t it takes the maximum of rows r..n-1 of its LDS column and tm[t * S + k].
// max is exact in any order, so this is the value the reference's scan finds, and it is a function of
// the lane's own column only: stream k's result does not depend on S. Cost: the input is read a second
// time, and 2 x 4 bytes per tile and stream of scratch traffic; a firing test costs at most BANK_F
// amplitudes, so a call stays O(frames) per stream.
#pragma once
#include "bank_kernels.h"
#include "loop_steps.h"

namespace sdrgpu {

// grid of tiles x waves folded into x (gridDim.y stops at 65535): block b is wave b % waves of tile b / waves
__device__ __forceinline__ void bank_tile_of_block(int S, int& t, int& k) {
    const int waves = (S + BANK_W - 1) / BANK_W;
    t = blockIdx.x / waves;
    k = (blockIdx.x % waves) * BANK_W + threadIdx.x;
}

// The walk of bank_fast_agc_kernel with the step handed in: step(x, t, r, n) is the output of row r (of
// n) of tile t, called in row order; X is the lane's tile (column threadIdx.x).
template <typename DT, typename Step>
__device__ __forceinline__ void bank_walk(DT* X, const DT* __restrict__ in, DT* __restrict__ out, int frames, int S,
                                          int k, Step step) {
    for (int m0 = 0, t = 0; m0 < frames; m0 += BANK_F, t++) {
        const int n = min(BANK_F, frames - m0);
        bank_stage(X, in, m0, n, S, k);
        DT* o = out + (size_t)m0 * S + k;
        for (int r = 0; r < n; r++) o[(size_t)r * S] = step(X[r * BANK_W + threadIdx.x], t, r, n);
    }
}

// ---------------------------------------------------------------------- AGC
// tm[t * S + k] = max |x| over the rows of tile t of stream k (exact)
template <typename DT>
__global__ __launch_bounds__(BANK_W) void bank_tile_max_kernel(const DT* __restrict__ in, int frames, int S, float* __restrict__ tm) {
    int t, k;
    bank_tile_of_block(S, t, k);
    if (k >= S) return;
    const int m0 = t * BANK_F, n = min(BANK_F, frames - m0);
    const DT* src = in + (size_t)m0 * S + k;
    float m = 0.0f;
    for (int r = 0; r < n; r++) m = fmaxf(m, amp_of(src[(size_t)r * S]));
    tm[(size_t)t * S + k] = m;
}

// state: amp[S], gain[S]. tm: the tile maxima on entry (enabled only). latch: AGC::setGain (agc.h:31)
// since the last call, for every stream.
template <typename DT>
__global__ __launch_bounds__(BANK_W) void bank_agc_kernel(const DT* __restrict__ in, DT* __restrict__ out, int frames, int S,
                                                          AgcParams p, float* __restrict__ st, float* tm, int latch, float latched) {
    __shared__ DT X[BANK_F * BANK_W];
    const int k = blockIdx.x * BANK_W + threadIdx.x;
    if (k >= S) return;
    float amp = st[k], gain = st[S + k];
    if (latch) gain = latched;
    if (p.enabled) {
        float run = 0.0f;   // tm[t] <- max over tiles > t (the look-ahead beyond tile t)
        for (int t = (frames + BANK_F - 1) / BANK_F - 1; t >= 0; t--) {
            const float v = tm[(size_t)t * S + k];
            tm[(size_t)t * S + k] = run;
            run = fmaxf(run, v);
        }
        bank_walk(X, in, out, frames, S, k, [&](DT x, int t, int r, int n) {
            const float g = agc_step(p, amp_of(x), amp, gain, [&] {
                float m = tm[(size_t)t * S + k];
                for (int q = r; q < n; q++) m = fmaxf(m, amp_of(X[q * BANK_W + threadIdx.x]));
                return m;
            });
            return scale_of(x, g);
        });
    } else {
        bank_walk(X, in, out, frames, S, k, [&](DT x, int, int, int) { return scale_of(x, agc_fixed_step(p, amp_of(x), gain)); });
    }
    st[k] = amp;
    st[S + k] = gain;
}

// ------------------------------------------------------------------ DCBlocker
// state: offset[S] (C64: re[S], im[S])
template <typename DT>
__global__ __launch_bounds__(BANK_W) void bank_dcb_kernel(const DT* __restrict__ in, DT* __restrict__ out, int frames, int S, float rate,
                                                          float* __restrict__ st) {
    __shared__ DT X[BANK_F * BANK_W];
    const int k = blockIdx.x * BANK_W + threadIdx.x;
    if (k >= S) return;
    float2 off = make_float2(st[k], 0.0f);
    if constexpr (sizeof(DT) == 8) off.y = st[S + k];
    bank_walk(X, in, out, frames, S, k, [&](DT x, int, int, int) { return dcb_step(x, off, rate); });
    st[k] = off.x;
    if constexpr (sizeof(DT) == 8) st[S + k] = off.y;
}

// ----------------------------------------------------------------- Deemphasis
// per channel (C = 1: float, DT = float; C = 2: stereo_t, DT = float2 = (l, r)), as deemp_kernel<C>;
// state: lastOut[S] (C = 2: l[S], r[S])
template <int C, typename DT>
__global__ __launch_bounds__(BANK_W) void bank_deemp_kernel(const DT* __restrict__ in, DT* __restrict__ out, int frames, int S,
                                                            float alpha, float* __restrict__ st) {
    static_assert(sizeof(DT) == 4 * C, "one float per channel");
    __shared__ DT X[BANK_F * BANK_W];
    const int k = blockIdx.x * BANK_W + threadIdx.x;
    if (k >= S) return;
    const float beta = 1 - alpha;                               // (1 - alpha): int - float -> float
    if constexpr (C == 1) {
        float last = st[k];
        bank_walk(X, in, out, frames, S, k, [&](float x, int, int, int) { return deemp_step(alpha, beta, x, last); });
        st[k] = last;
    } else {
        float l = st[k], r = st[S + k];
        bank_walk(X, in, out, frames, S, k, [&](float2 x, int, int, int) {
            const float yl = deemp_step(alpha, beta, x.x, l);
            return make_float2(yl, deemp_step(alpha, beta, x.y, r));
        });
        st[k] = l;
        st[S + k] = r;
    }
}

// -------------------------------------------------------------------- Squelch
// The column sum of stream k (squelch.h:35-36), in an order that depends on `frames` alone: the rows of
// every BANK_F-row tile are added in ascending order from 0 (part[t * S + k], tiles x waves grid), then
// the tile sums in ascending order from 0 (the decision's lane). No atomics; S, the grid and the run do
// not enter.
__global__ __launch_bounds__(BANK_W) void bank_squelch_partial_kernel(const float2* __restrict__ in, int frames, int S,
                                                                      float* __restrict__ part) {
    int t, k;
    bank_tile_of_block(S, t, k);
    if (k >= S) return;
    const int m0 = t * BANK_F, n = min(BANK_F, frames - m0);
    const float2* src = in + (size_t)m0 * S + k;
    float sum = 0.0f;
    for (int r = 0; r < n; r++) sum += amp_of(src[(size_t)r * S]);
    part[(size_t)t * S + k] = sum;
}

// one lane per stream: the level and the mute state machine (squelch.h:37-53); state: muted[S], cnt[S]
__global__ __launch_bounds__(BANK_W) void bank_squelch_decide_kernel(const float* __restrict__ part, int frames, int S, float L,
                                                                     int* __restrict__ st) {
    const int k = blockIdx.x * BANK_W + threadIdx.x;
    if (k >= S) return;
    float sum = 0.0f;
    for (int t = 0; t < (frames + BANK_F - 1) / BANK_F; t++) sum += part[(size_t)t * S + k];
    sum /= (float)frames;
    const float level = 20.0f * log10f(sum);
    int muted = st[k], cnt = st[S + k];
    if (muted) {
        if (level < L || cnt <= 0) cnt = 10;        // 10 calls above the level before unmute
        else if (--cnt == 0) muted = 0;
    } else if (level < (L - 1.0f)) {                // 1 dB hysteresis
        cnt = 0;
        muted = 1;
    }
    st[k] = muted;
    st[S + k] = cnt;
}

// memset / memcpy per stream (squelch.h:55-60), coalesced over the flat stream
__global__ void bank_squelch_gate_kernel(const float2* __restrict__ in, float2* __restrict__ out, int n, int S,
                                         const int* __restrict__ muted) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // (the grid's last block may pass INT_MAX)
    if (i >= n) return;
    out[i] = muted[i % S] ? make_float2(0.f, 0.f) : in[i];
}

// ------------------------------------------------------------------ magnitude
// volk_32fc_magnitude_32f (am.h:121) does not know of rows: magnitude_kernel's expression over the flat stream
__global__ void bank_magnitude_kernel(const float2* __restrict__ in, float* __restrict__ out, int n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = amp_of(in[i]);
}

}  // namespace sdrgpu
