// Bit-exact recurrences: include this header only from a translation unit built with
// -ffp-contract=off (sdrpp_amd/build.py does that for bank.hip; symsync_kernels.h says why).
//
// Device code of bank.hip: stream banks. A bank is S independent streams in the channelizer's
// frame-major layout: element m of stream k is x[m * S + k] (chan_kernels.h writes out[m * M + k]).
//   demod::Quadrature, filter::FIR<D, float>      one thread per (row, stream), coalesced over streams
//   channel::FrequencyXlator                       one block per (row group, 256-stream chunk): the row's phasor is the block's
//   loop::FastAGC<T>, loop::Costas<ORDER>, loop::MeteorCostas,
//   loop::PLL, loop::CarrierTrackingPLL,
//   clock_recovery::MM<T>                          one lane per stream
//
// The lane-per-stream walk. A workgroup is one wave and owns BANK_W = 64 consecutive streams; lane l
// is stream k = 64 blockIdx.x + l. Lanes k >= S load and store no stream data and leave at once. The
// recurrences are the per-sample steps of symsync_kernels.h (fast_agc_step, costas_step, meteor_costas_step, mm_step;
// pll_step of loop_steps.h), so a
// bank column is the single-stream kernel's arithmetic. Per-stream state is structure-of-arrays
// (word f of stream k at st[f * S + k]): a wave's state load and store are coalesced.
//
// Rows come in ahead of the walk as an LDS tile X[BANK_F rows][64 streams]: the wave issues the tile's
// row loads back to back (each 256 B for F32, 512 B for C64, fully coalesced) and pays the global-load
// latency once per tile, not once per step. Lane l reads and writes column l only -- word r * 64 + l, i.e.
// bank l mod 32 for the 32 lanes an LDS cycle serves (F32; C64: dwords 2l, 2l + 1 of 64 banks) at any row,
// conflict-free also where MM's lanes sit at different rows -- and no lane reads what another wrote, so
// the walk has no barrier. Outputs go straight to global memory: the
// stores of a row are coalesced and nothing waits for them.
#pragma once
// quad_value is the expression of the single-stream quadrature, which blocks.hip compiles with the
// default contraction: the same contraction here gives the same bits (quad_value.h)
// (and xlate_value, the expression of the single-stream frequency xlator: nco_value.h)
#pragma clang fp contract(fast)
#include "quad_value.h"
#include "nco_value.h"
#pragma clang fp contract(off)
#include "symsync_kernels.h"

namespace sdrgpu {

constexpr int BANK_W = 64;   // streams per wave (= per workgroup)
constexpr int BANK_F = 32;   // rows per LDS tile: 8 KiB (F32) / 16 KiB (C64) per workgroup; MM adds T - 1 rows and its bank

// rows [m0, m0 + n) of column k into the tile (n <= BANK_F); the full tile's loads are unrolled so that
// all of them are in flight together
template <typename DT>
__device__ __forceinline__ void bank_stage(DT* __restrict__ X, const DT* __restrict__ in, int m0, int n, int S, int k) {
    const DT* src = in + (size_t)m0 * S + k;
    DT* dst = X + threadIdx.x;
    if (n == BANK_F) {
#pragma unroll
        for (int r = 0; r < BANK_F; r++) dst[r * BANK_W] = src[(size_t)r * S];
    } else {
        for (int r = 0; r < n; r++) dst[r * BANK_W] = src[(size_t)r * S];
    }
}

// ------------------------------------------------------------------ FastAGC
// state: gain[S]
template <typename DT>
__global__ __launch_bounds__(BANK_W) void bank_fast_agc_kernel(const DT* __restrict__ in, DT* __restrict__ out, int frames, int S,
                                                               FastAgcParams p, float* __restrict__ st) {
    __shared__ DT X[BANK_F * BANK_W];
    const int k = blockIdx.x * BANK_W + threadIdx.x;
    if (k >= S) return;
    float gain = st[k];
    for (int m0 = 0; m0 < frames; m0 += BANK_F) {
        const int n = min(BANK_F, frames - m0);
        bank_stage(X, in, m0, n, S, k);
        DT* o = out + (size_t)m0 * S + k;
        for (int r = 0; r < n; r++) o[(size_t)r * S] = fast_agc_step(p, X[r * BANK_W + threadIdx.x], gain);
    }
    st[k] = gain;
}

// ------------------------------------------------------------------- Costas
// state: phase[S], freq[S]
template <int ORDER>
__global__ __launch_bounds__(BANK_W) void bank_costas_kernel(const float2* __restrict__ in, float2* __restrict__ out, int frames,
                                                             int S, PclParams p, float* __restrict__ st) {
    __shared__ float2 X[BANK_F * BANK_W];
    const int k = blockIdx.x * BANK_W + threadIdx.x;
    if (k >= S) return;
    float phase = st[k], freq = st[S + k];
    for (int m0 = 0; m0 < frames; m0 += BANK_F) {
        const int n = min(BANK_F, frames - m0);
        bank_stage(X, in, m0, n, S, k);
        float2* o = out + (size_t)m0 * S + k;
        for (int r = 0; r < n; r++) o[(size_t)r * S] = costas_step<ORDER>(p, X[r * BANK_W + threadIdx.x], phase, freq);
    }
    st[k] = phase;
    st[S + k] = freq;
}

// ------------------------------------------------------------- MeteorCostas
// state: phase[S], freq[S]; lastI[S] apart from it (a reset keeps it), read and written only while the
// stagger is on
static __global__ __launch_bounds__(BANK_W) void bank_meteor_costas_kernel(const float2* __restrict__ in, float2* __restrict__ out,
                                                                          int frames, int S, PclParams p, int broken, int oqpsk,
                                                                          float* __restrict__ st, float* __restrict__ lastIs) {
    __shared__ float2 X[BANK_F * BANK_W];
    const int k = blockIdx.x * BANK_W + threadIdx.x;
    if (k >= S) return;
    float phase = st[k], freq = st[S + k];
    float lastI = oqpsk ? lastIs[k] : 0.0f;
    for (int m0 = 0; m0 < frames; m0 += BANK_F) {
        const int n = min(BANK_F, frames - m0);
        bank_stage(X, in, m0, n, S, k);
        float2* o = out + (size_t)m0 * S + k;
        for (int r = 0; r < n; r++) {
            const float2 y = meteor_costas_step(p, broken, X[r * BANK_W + threadIdx.x], phase, freq);
            o[(size_t)r * S] = oqpsk ? oqpsk_stagger(y, lastI) : y;
        }
    }
    st[k] = phase;
    st[S + k] = freq;
    if (oqpsk) lastIs[k] = lastI;
}

// ------------------------------------------------- PLL, CarrierTrackingPLL
// state: phase[S], freq[S]
template <bool DEROTATE>
__global__ __launch_bounds__(BANK_W) void bank_carrier_pll_kernel(const float2* __restrict__ in, float2* __restrict__ out, int frames,
                                                                  int S, PllParams p, float* __restrict__ st) {
    __shared__ float2 X[BANK_F * BANK_W];
    const int k = blockIdx.x * BANK_W + threadIdx.x;
    if (k >= S) return;
    float phase = st[k], freq = st[S + k];
    for (int m0 = 0; m0 < frames; m0 += BANK_F) {
        const int n = min(BANK_F, frames - m0);
        bank_stage(X, in, m0, n, S, k);
        float2* o = out + (size_t)m0 * S + k;
        for (int r = 0; r < n; r++) {
            const float2 v = X[r * BANK_W + threadIdx.x];
            const float vco = pll_step(p, atan2f(v.y, v.x), phase, freq);
            o[(size_t)r * S] = pll_output<DEROTATE>(v, vco);
        }
    }
    st[k] = phase;
    st[S + k] = freq;
}

// ----------------------------------------------------------------------- MM
// state words (int or float bits), word f of stream k at st[f * S + k]
enum MmWord {
    MMW_OFFSET, MMW_PHASE, MMW_FREQ, MMW_LAST_OUT,                       // MmState::offset .. lastOut
    MMW_P0, MMW_P1 = MMW_P0 + 2, MMW_P2 = MMW_P1 + 2,                    // MM<complex_t>: (x, y) pairs
    MMW_C0 = MMW_P2 + 2, MMW_C1 = MMW_C0 + 2, MMW_C2 = MMW_C1 + 2,
    MMW_COUNT = MMW_C2 + 2,                                              // outputs of the last call
    MMW_WORDS
};
__device__ __forceinline__ float2 mmw_pair(const int* st, int f, int S, int k) {
    return make_float2(__int_as_float(st[(f)*S + k]), __int_as_float(st[(f + 1) * S + k]));
}
__device__ __forceinline__ void mmw_put(int* st, int f, int S, int k, float2 v) {
    st[f * S + k] = __float_as_int(v.x);
    st[(f + 1) * S + k] = __float_as_int(v.y);
}

// tap j of interpolator phase ph in the LDS copy. A 4-byte LDS read serves 32 lanes per cycle over 32
// banks. Transposed (tap-major): at tap j the lanes' words are j P + ph_l, so two lanes of a group conflict
// only where their phases differ and are equal mod 32 (4-way at most for P = 128; equal phases broadcast).
// Row-major (ph T + j, SDRGPU_BANK_INTERP_ROWMAJOR, for the A/B measurement) puts a tap's words of all
// phases on 32 / T banks: with T = 8, 4 banks, 8-way once a group's lanes sit at 32 different phases.
// Measured: tap-major 5 % (float) / 2 % (complex) faster per call on noise.
__device__ __forceinline__ int interp_word(int ph, int j, int P, int T) {
#ifdef SDRGPU_BANK_INTERP_ROWMAJOR
    return ph * T + j;
#else
    return j * P + ph;
#endif
}

// The work buffer of stream k is [hist (T - 1 rows) || in (frames rows)], both in the bank layout. A
// tile stages work rows [i0, i0 + n + T - 1); a lane makes the outputs whose offset falls in [i0, i0 + n),
// at most n of them (mm_kernel's bounds: every output consumes an input, and a NaN in one stream's loop
// cannot hold the wave's other streams). Output j of stream k goes to out[j * S + k]; the lanes' trip
// counts differ by a few, the wave runs the longest. The interpolator bank (shared parameters, not
// stream data) is copied to LDS by all 64 lanes before the lanes past S leave.
// Dynamic LDS: (BANK_F + T - 1) * 64 elements, then the P * T bank where it fits MM_LDS_BANK.
template <typename DT>
__global__ __launch_bounds__(BANK_W) void bank_mm_kernel(const DT* __restrict__ in, int frames, int S, DT* __restrict__ out,
                                                         MmParams p, const float* __restrict__ bank, DT* __restrict__ hist,
                                                         int* __restrict__ st) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bank_mm_lds[];
    const int l = threadIdx.x, k = blockIdx.x * BANK_W + l;
    const int T = p.T, H = p.T - 1, P = p.P;
    DT* W = reinterpret_cast<DT*>(bank_mm_lds);
    float* BL = reinterpret_cast<float*>(W + (BANK_F + H) * BANK_W);
    const bool bankLds = P * T <= MM_LDS_BANK;
    if (bankLds) {
        for (int i = l; i < P * T; i += BANK_W) BL[interp_word(i / T, i % T, P, T)] = bank[i];
        __syncthreads();
    }
    if (k >= S) return;
    MmState s{};
    s.offset = st[MMW_OFFSET * S + k];
    s.phase = __int_as_float(st[MMW_PHASE * S + k]);
    s.freq = __int_as_float(st[MMW_FREQ * S + k]);
    if constexpr (sizeof(DT) == 4) {
        s.lastOut = __int_as_float(st[MMW_LAST_OUT * S + k]);
    } else {
        s.p0 = mmw_pair(st, MMW_P0, S, k); s.p1 = mmw_pair(st, MMW_P1, S, k); s.p2 = mmw_pair(st, MMW_P2, S, k);
        s.c0 = mmw_pair(st, MMW_C0, S, k); s.c1 = mmw_pair(st, MMW_C1, S, k); s.c2 = mmw_pair(st, MMW_C2, S, k);
    }
    // work row w of this column
    auto work = [&](int w) -> DT { return w < H ? hist[(size_t)w * S + k] : in[(size_t)(w - H) * S + k]; };
    int outBase = 0;
    for (int i0 = 0; i0 < frames; i0 += BANK_F) {
        const int n = min(BANK_F, frames - i0);
        if (i0 >= H && n == BANK_F) {   // (past the history rows: plain loads, all in flight)
            const DT* src = in + (size_t)(i0 - H) * S + k;
            for (int e = 0; e < BANK_F + H; e++) W[e * BANK_W + l] = src[(size_t)e * S];
        } else {
            for (int e = 0; e < n + H; e++) W[e * BANK_W + l] = work(i0 + e);
        }
        int no = 0;
        auto walk = [&](auto b) {
            while (s.offset >= i0 && s.offset < i0 + n && no < n) {
                const DT* x = &W[(s.offset - i0) * BANK_W + l];
                out[(size_t)(outBase + no) * S + k] = mm_step<DT>(p, s, [&](int j) { return x[j * BANK_W]; }, b);
                no++;
            }
        };
        if (bankLds) walk([&](int ph, int j) { return BL[interp_word(ph, j, P, T)]; });
        else walk([&](int ph, int j) { return bank[ph * T + j]; });
        outBase += no;
    }
    // mm.h:150-153: offset -= count; the last T - 1 work rows become the history. A lane owns its column
    // and moves it in ascending rows: row t is written after row frames + t > t was read.
    for (int t = 0; t < H; t++) {
        const DT v = work(frames + t);
        hist[(size_t)t * S + k] = v;
    }
    st[MMW_OFFSET * S + k] = s.offset - frames;
    st[MMW_PHASE * S + k] = __float_as_int(s.phase);
    st[MMW_FREQ * S + k] = __float_as_int(s.freq);
    if constexpr (sizeof(DT) == 4) {
        st[MMW_LAST_OUT * S + k] = __float_as_int(s.lastOut);
    } else {
        mmw_put(st, MMW_P0, S, k, s.p0); mmw_put(st, MMW_P1, S, k, s.p1); mmw_put(st, MMW_P2, S, k, s.p2);
        mmw_put(st, MMW_C0, S, k, s.c0); mmw_put(st, MMW_C1, S, k, s.c1); mmw_put(st, MMW_C2, S, k, s.c2);
    }
    st[MMW_COUNT * S + k] = outBase;
}

// ----------------------------------------------- quadrature, FIR: data-parallel
// In the bank layout the S streams are one flat stream of S-vectors: the sample before element i is
// element i - S, so these kernels are the single-stream ones with the lag scaled by S, one thread per
// element i = m S + k, coalesced over k.
//
// demod/quadrature.h:41-56 per stream; prev[k]: the last sample of the previous call (quad_kernel's din)
__global__ void bank_quad_kernel(const float2* __restrict__ in, float* __restrict__ out, int n, int S,
                                 const float2* __restrict__ prev, float2* __restrict__ prevNext, float invDev) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // (the grid's last block may pass INT_MAX)
    if (i >= n) return;
    const float2 y = in[i];
    out[i] = quad_value(y, i >= S ? in[i - S] : prev[i], invDev);
    if (i >= n - S) prevNext[i - (n - S)] = y;
}

// (bank_fir_kernel, filter/fir.h:60-80 per stream, is in symsync_kernels.h: the single-stream Meteor chain runs it too, S = 1)

// ------------------------------------------------------------------- xlator
// channel/frequency_xlator.h:43-50 per stream, one NCO for the bank: out[m S + k] = in[m S + k] * nco(m),
// the phasor of row m being nco_tab(phi, plo, m) of the single-stream NCO's tables for a call of `frames`
// samples (xlate_value: xlator_kernel's expression, so column k is a single-stream handle fed column k).
// All S elements of a row share the phasor, so the row is the block's, not the thread's: block b is
// the 256-stream chunk b % chunks of the BANK_XR-row group b / chunks (one 32-bit scalar division per
// block, the pair folded into grid.x as bank_tile_of_block), thread t is stream k = 256 chunk + t in every
// row of the group. The row index is uniform over the block: the two table reads have a uniform address
// (scalar loads; 16 bytes per wave and row, against 64 x 8 of samples), and the element index is a
// uniform 64-bit m S plus k: no per-element division by S. A wave's 64 loads and stores of a row are
// consecutive 8-byte (C64) or 4-byte (REAL out) words; the group's BANK_XR loads are unrolled and in
// flight together. Traffic per element: 8 B read, 8 B written; REAL keeps the real component (the real
// part of the same product: 8 B read, 4 B written, in place of 16 + 12 for the xlator and a real-part pass).
constexpr int BANK_XR = 8;     // rows per block
constexpr int BANK_XS = 256;   // streams per block (= threads)
template <bool REAL>
__global__ __launch_bounds__(BANK_XS) void bank_xlate_kernel(const float2* __restrict__ in, void* __restrict__ outv, int frames, int S,
                                                             int chunks, const float2* __restrict__ phi,
                                                             const float2* __restrict__ plo) {
    const int g = blockIdx.x / chunks;
    const int k = (blockIdx.x - g * chunks) * BANK_XS + threadIdx.x;
    if (k >= S) return;
    const int m0 = g * BANK_XR, n = min(BANK_XR, frames - m0);
    const float2* src = in + (size_t)m0 * S + k;
    // Rows past the group's last reread it, so the loads are unconditional; each value is then pinned to its
    // VGPRs (as xlate_slot does, fir_rows.h), or the compiler sinks every load into its row's branch below and
    // the group becomes load, wait, store eight times over.
    float2 x[BANK_XR];
#pragma unroll
    for (int r = 0; r < BANK_XR; r++) x[r] = src[(size_t)min(r, n - 1) * S];
#pragma unroll
    for (int r = 0; r < BANK_XR; r++) asm volatile("" : "+v"(x[r].x), "+v"(x[r].y));
#pragma unroll
    for (int r = 0; r < BANK_XR; r++) {
        if (r >= n) break;
        const float2 y = xlate_value(x[r], phi, plo, m0 + r);
        const size_t o = (size_t)(m0 + r) * S + k;
        if constexpr (REAL) reinterpret_cast<float*>(outv)[o] = y.x;
        else reinterpret_cast<float2*>(outv)[o] = y;
    }
}

}  // namespace sdrgpu
