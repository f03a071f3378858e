// Bit-exact sums and recurrences: include this header only from a translation unit built with
// -ffp-contract=off (sdrpp_amd/build.py does that for bank.hip; bank_kernels.h says why).
//
// Device code of the broadcast-FM bank of bank.hip, in the bank layout, element m of stream k
// at x[m * S + k]; stereo_t is float2 (l, r):
//   filter::FIR<complex_t, complex_t>     filter/fir.h:75 (volk_32fc_x2_dot_prod_32fc) per stream, complex taps
//   loop::PLL                             loop/pll.h:64-70, one lane per stream (pll_step, loop_steps.h)
//   the stereo matrix, mono -> pairs      demod/broadcast_fm.h:173-190, :211, one thread per (row, stream)
//
// The complex-tap FIR. Over the work rows [hist (T - 1 rows) || in] of stream k, taps not reversed:
//   out[j * S + k] = sum_t work_k[j + t] * taps[t],  per tap, in ascending t, fp32, unfused:
//     re += (x.re * t.re) - (x.im * t.im)
//     im += (x.re * t.im) + (x.im * t.re)
// A sum of row j reads rows j .. j + T - 1 only, so it does not depend on how the rows are cut into calls.
// Real input (IN = float) is convert::RealToComplex followed by the filter (broadcast_fm.h:149-152) in one
// launch, at half the input traffic: x.im = 0, and per tap
//     re += x * t.re
//     im += x * t.im
// which has the bits of the complex expression for finite taps: 0 * t is then +-0; added to or subtracted from a
// non-zero product it changes nothing, and where the product is itself +-0 the term is +-0 either way, which an
// accumulator that is never -0 (it starts at +0, and a sum is -0 only where both terms are) takes unchanged.
// PHASE: the output is atan2f(y.im, y.re) (F32), phase_kernel's expression (complex_t::phase(), types.h:57): what
// the PLL reads, so the stereo decoder never stores the filtered pilot.
//
// Two forms with the same sum, hence the same bits (the forms of bank_rate_kernels.h):
//   direct  one thread per output element, block = one row x 256 streams; the work rows come from global memory
//           (hist / in), each input element T times, out of L2. The baseline of the bits.
//   tiled   a workgroup of 8 waves owns 64 streams x R output rows (CfirArgs::R <= 64, cfir_tile on the host) and
//           stages work rows as X[row][64 lanes] in LDS: a lane reads column l only, word r * 64 + l (C64: dwords
//           2l, 2l + 1), conflict-free at any row. Wave w makes rows w, w + 8, ... of the R, their sums in registers
//           (CFIR_RPW accumulators). The staged rows fit CFIR_LDS = 64 KiB (two workgroups per CU of 160 KiB): 256
//           rows of F32, 128 of C64. The 305 pilot taps at 240 kS/s need R + 304 rows, more than either, so the
//           taps are taken in segments of Tc (CfirArgs::Tc): per segment t0 the workgroup stages rows j0 + t0 ..
//           j0 + t0 + n + tc - 2 and every sum advances over taps t0 .. t0 + tc - 1, still in ascending tap order,
//           so the bits do not depend on R or Tc. T <= Tc is one segment: rows first .. last + T - 1 staged once.
//           Global reads per input element: segments * (R + Tc - 1) / R. A call with few rows takes smaller tiles,
//           as many as give CFIR_WGS workgroups, one row per wave at least; below CFIR_RMIN rows it runs direct.
// Tap pairs are read at a uniform address (scalar loads) in both forms.
// Bounds: the last work row read is M - 1 + T - 1 < M + H = the rows of [hist || in]; k < S is checked before any
// access to stream data; the tile's last LDS row is n + tc - 2 < R + Tc - 1 = the rows the host sized.
#pragma once
#include "bank_audio_kernels.h"   // bank_kernels.h (BANK_W, BANK_F, bank_stage), loop_steps.h
#include "bank_rate_kernels.h"    // rate_work

namespace sdrgpu {

constexpr int CFIR_W = 64;              // streams per tiled workgroup (lanes of a wave)
constexpr int CFIR_TW = 8;              // waves per tiled workgroup
constexpr int CFIR_RPW = 8;             // output rows per wave and tile at most: R <= CFIR_TW * CFIR_RPW = 64
constexpr int CFIR_XS = 256;            // streams per direct block (= threads)
constexpr int CFIR_LDS = 64 * 1024;     // LDS bytes of a tile at most
constexpr int CFIR_RMIN = 4;            // a call below this many rows runs the direct kernel
constexpr int CFIR_WGS = 512;           // workgroups a call aims for before its tiles grow past a row per wave (2 per CU)

struct CfirArgs {
    int S, H, T;           // streams, history rows (T - 1), taps
    int M, R, Tc, chunks;  // rows of the call; rows per tile and taps per segment (tiled); stream chunks per row (group)
};

__device__ __forceinline__ void cfir_mac(float2& acc, float x, float2 t) {
    acc.x += x * t.x;
    acc.y += x * t.y;
}
__device__ __forceinline__ void cfir_mac(float2& acc, float2 x, float2 t) {
    acc.x += (x.x * t.x) - (x.y * t.y);
    acc.y += (x.x * t.y) + (x.y * t.x);
}
template <bool PHASE>
__device__ __forceinline__ void cfir_put(void* __restrict__ outv, size_t i, float2 y) {
    if constexpr (PHASE) reinterpret_cast<float*>(outv)[i] = atan2f(y.y, y.x);
    else reinterpret_cast<float2*>(outv)[i] = y;
}

// direct: block b is the 256-stream chunk b % chunks of output row b / chunks
template <typename IN, bool PHASE>
__global__ __launch_bounds__(CFIR_XS) void bank_cfir_direct_kernel(const IN* __restrict__ hist, const IN* __restrict__ in,
                                                                   const float2* __restrict__ taps, void* __restrict__ outv,
                                                                   CfirArgs a) {
    const int j = blockIdx.x / a.chunks;
    const int k = (blockIdx.x - j * a.chunks) * CFIR_XS + threadIdx.x;
    if (k >= a.S) return;
    float2 acc{};
#pragma unroll 4
    for (int t = 0; t < a.T; t++) cfir_mac(acc, rate_work(hist, in, j + t, a.H, a.S, k), taps[t]);
    cfir_put<PHASE>(outv, (size_t)j * a.S + k, acc);
}

// tiled: block b is the 64-stream chunk b % chunks of the R-row group b / chunks.
// Dynamic LDS: (R + Tc - 1) * 64 elements of IN, at most CFIR_LDS bytes (cfir_tile). Every thread reaches
// every barrier: the lanes past S only skip the accesses.
template <typename IN, bool PHASE>
__global__ __launch_bounds__(CFIR_TW* CFIR_W) void bank_cfir_tiled_kernel(const IN* __restrict__ hist, const IN* __restrict__ in,
                                                                          const float2* __restrict__ taps, void* __restrict__ outv,
                                                                          CfirArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bank_cfir_lds[];
    IN* X = reinterpret_cast<IN*>(bank_cfir_lds);
    const int g = blockIdx.x / a.chunks;
    const int l = threadIdx.x & (CFIR_W - 1);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / CFIR_W));
    const int k = (blockIdx.x - g * a.chunks) * CFIR_W + l;
    const bool live = k < a.S;
    const int j0 = g * a.R, n = min(a.R, a.M - j0);
    float2 acc[CFIR_RPW];
#pragma unroll
    for (int i = 0; i < CFIR_RPW; i++) acc[i] = make_float2(0.0f, 0.0f);
    for (int t0 = 0; t0 < a.T; t0 += a.Tc) {
        const int tc = min(a.Tc, a.T - t0);
        const int nr = n + tc - 1;   // staged rows of this segment
        if (t0 > 0) __syncthreads();   // (the previous segment's rows have been read)
        if (live) {
#pragma unroll 4
            for (int r = wv; r < nr; r += CFIR_TW) X[r * CFIR_W + l] = rate_work(hist, in, j0 + t0 + r, a.H, a.S, k);
        }
        __syncthreads();
        if (live) {
            const float2* hb = taps + t0;
#pragma unroll
            for (int i = 0; i < CFIR_RPW; i++) {
                const int r = wv + i * CFIR_TW;
                if (r < n) {
                    const IN* x = X + r * CFIR_W + l;
                    float2 c = acc[i];
#pragma unroll 8
                    for (int t = 0; t < tc; t++) cfir_mac(c, x[t * CFIR_W], hb[t]);
                    acc[i] = c;
                }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int i = 0; i < CFIR_RPW; i++) {
        const int r = wv + i * CFIR_TW;
        if (r < n) cfir_put<PHASE>(outv, (size_t)(j0 + r) * a.S + k, acc[i]);
    }
}

// ------------------------------------------------------------------------ PLL
// The lane-per-stream walk of bank_kernels.h on pll_step, in place on the phase plane: th[m * S + k] = the
// phase of the filtered pilot -> the phase the VCO outputs for row m (BEFORE the advance, pll.h:66-67). The
// recurrence alone: atan2f is the FIR's epilogue, cosf / sinf the matrix's. A tile's rows are loaded (bank_stage)
// before any of them is stored, and no row is loaded twice. At S = 1024 this is 16 waves of 1024 dependent steps,
// the longest launch of the decoder. state: phase[S], freq[S]
__global__ __launch_bounds__(BANK_W) void bank_pll_kernel(float* th, int frames, int S, PllParams p, float* __restrict__ st) {
    __shared__ float X[BANK_F * BANK_W];
    const int k = blockIdx.x * BANK_W + threadIdx.x;
    if (k >= S) return;
    float phase = st[k], freq = st[S + k];
    for (int m0 = 0; m0 < frames; m0 += BANK_F) {
        const int n = min(BANK_F, frames - m0);
        bank_stage(X, th, m0, n, S, k);
        float* o = th + (size_t)m0 * S + k;
        if (n == BANK_F) {   // a full tile: the column into registers with one wait, so that a step waits for no LDS read
            float v[BANK_F];
#pragma unroll
            for (int r = 0; r < BANK_F; r++) v[r] = X[r * BANK_W + threadIdx.x];
#pragma unroll
            for (int r = 0; r < BANK_F; r++) o[(size_t)r * S] = pll_step(p, v[r], phase, freq);
        } else {
            for (int r = 0; r < n; r++) o[(size_t)r * S] = pll_step(p, X[r * BANK_W + threadIdx.x], phase, freq);
        }
    }
    st[k] = phase;
    st[S + k] = freq;
}

// ------------------------------------------------- matrix, mono -> pairs: data-parallel
// stereo_matrix_kernel (loop_kernels.h) over the flat stream of S-vectors, as bank_quad_kernel: the MPX `delay`
// rows back is element i - DS of [hist (DS = delay * S elements) || mpx]; n = frames * S. The history carry is
// carry_history (blocks.h) over the flat stream.
__global__ void bank_stereo_matrix_kernel(const float* __restrict__ mpx, const float* __restrict__ hist, int DS,
                                          const float* __restrict__ vcoPhase, float2* __restrict__ lr, int n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // (the grid's last block may pass INT_MAX)
    if (i >= n) return;
    const float d = i < DS ? hist[i] : mpx[i - DS];             // Delay<float> / Delay<complex_t>.re
    lr[i] = stereo_matrix_value(d, vcoPhase[i]);
}

// convert::MonoToStereo (broadcast_fm.h:211): l = r, mono_to_stereo_kernel's expression over the flat stream
__global__ void bank_mono_pairs_kernel(const float* __restrict__ in, float2* __restrict__ out, int n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = make_float2(in[i], in[i]);
}

}  // namespace sdrgpu
