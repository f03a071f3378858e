// The FIR tile kernel of the channel chain (blocks.hip FirBlock, the VALU path): any data / tap type
// pair, any decimation, with the frequency xlator optionally fused into its load and the FM quadrature
// or the LRToStereo interleave into its store.
#pragma once
#include "fir_rows.h"

namespace sdrgpu {

// ------------------------------------------------------------ FIR engine
// out[m] = sum_{j<ntaps} buf[offset0 + m*D + j] * taps[j],  buf = hist(H) | in(count)
// (correlation order, filter/fir.h:62-83, decimating_fir.h:45-68).
// LDS holds one tile's input span "phase-major": span element s goes to phase
// p = s % D, row r = s / D, at p*RSP + (r % K)*RSK + r / K. Thread l computes K
// consecutive outputs from a K-deep register window that slides one row per tap
// step, so lanes read consecutive LDS words (conflict-free for any D) and every
// row load feeds K outputs.


// FIR tile kernel: one tile of NT*K outputs per workgroup.
//  1. The tile's input span (rows * D elements) is loaded with all PF loads per thread in
//     flight at once (interior tiles; the few tiles touching the history or the tail of the
//     call fetch element-wise), the fused xlator's NCO phasor is formed as
//     base(tid) * S[u] (S[u] = e^{i w u NT}, wave-uniform scalar loads) instead of two table
//     loads per element, and each element is stored into the phase-major, row-swizzled LDS
//     image X[p][r % K][r / K] with an address that advances by a constant per slot when
//     D | NT and K | NT/D (all plan stages), else with the general index split.
//  2. Each thread computes K consecutive outputs with a register window sliding one row per
//     tap; taps are staged once per workgroup in LDS (wave-uniform broadcast reads).
// History / tail samples come from [hist (H) || in (count)]; hist is stored translated.


template <typename DT, typename TT, int K, bool XL, bool QUAD, bool STEREO, bool TL>
__global__ __launch_bounds__(256) void fir_kernel(FirArgs a) {
    if (fir_hist_block<DT, XL>(a)) return;
    constexpr int PF = sizeof(DT) == 8 ? 36 : 40;   // load slots per thread issued together
    const int NT = blockDim.x;       // 64, 128 or 256 (host picks the largest tile that fits LDS)
    const int TM = NT * K;
    constexpr int QOFF = QUAD ? 1 : 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    DT* X = reinterpret_cast<DT*>(smem);
    __shared__ float2 lastY[QUAD ? 256 : 1];

    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const int rows = TM + a.Q + K;                               // padded taps + prefetch rows
    const int span = rows * a.D;
    const DT* in = reinterpret_cast<const DT*>(a.in);
    const TT* __restrict__ taps = reinterpret_cast<const TT*>(a.taps);
    if constexpr (TL) {
        TT* tl = reinterpret_cast<TT*>(smem + a.tapsLdsOff);
        for (int i = tid; i < a.D * a.Q; i += NT) tl[i] = taps[i];
        taps = tl;                                                // (ordered by the barrier below)
    }
    auto lds_index = [&](int sx) {
        int p, r;
        if (a.dshift >= 0) {
            p = sx & (a.D - 1);
            r = sx >> a.dshift;
        } else {
            r = sx / a.D;
            p = sx - r * a.D;
        }
        return p * a.RSP + (r % K) * a.RSK + r / K;
    };

    const int mFirst = tile * a.TMS - QOFF;                      // output of local index 0
    const long long b0 = (long long)a.offset0 + (long long)mFirst * a.D;
    const bool interior = (b0 >= a.H) && (b0 + span <= (long long)a.H + a.count);
    int sxRest = tid;                                            // first slot fetched element-wise
    if (interior) {
        const DT* __restrict__ src = in + (b0 - a.H);
        DT pf[PF];
#pragma unroll
        for (int u = 0; u < PF; u++) {
            const int sx = tid + u * NT;
            if (sx < span) pf[u] = src[sx];
        }
        if constexpr (XL) {
            // phasor(i0 + tid + u NT) = nco(i0 + tid) * e^{i w u NT}
            const float2 ph0 = nco_at(a, b0 - a.H + tid);
            const float2* __restrict__ S = a.nstep;
#pragma unroll
            for (int u = 0; u < PF; u++) pf[u] = xlate_slot(pf[u], ph0, S[u]);
        }
        if (a.simple) {
            // D | NT and K | NT/D: the slot's phase is fixed, its row advances by NT/D
            int idx = lds_index(tid);
            const int inc = (NT / a.D) / K;
#pragma unroll
            for (int u = 0; u < PF; u++) {
                if (tid + u * NT < span) X[idx] = pf[u];
                idx += inc;
            }
        } else {
#pragma unroll
            for (int u = 0; u < PF; u++) {
                const int sx = tid + u * NT;
                if (sx < span) X[lds_index(sx)] = pf[u];
            }
        }
        sxRest = tid + PF * NT;                                  // remainder (rare: huge decimations)
    }
    for (int sx = sxRest; sx < span; sx += NT) X[lds_index(sx)] = fir_fetch<DT, XL>(a, b0 + sx);
    __syncthreads();

    DT acc[K];
#pragma unroll
    for (int i = 0; i < K; i++) acc[i] = zero_of<DT>();
    // a.Q is padded to a multiple of QC with zero taps. Row l*K + j + K*s of phase p sits at
    // Xj[j][s] (j = row % K), so a chunk's QC row reads are K base addresses + immediates.
    constexpr int QC = 8;
    const int l = tid;
    for (int p = 0; p < a.D; p++) {
        const DT* Xj[K];
#pragma unroll
        for (int j = 0; j < K; j++) Xj[j] = X + p * a.RSP + j * a.RSK + l;
        const TT* __restrict__ Hp = taps + p * a.Q;
        DT w[K];
#pragma unroll
        for (int i = 0; i < K; i++) w[i] = Xj[i][0];                // rows l*K + i
        // (unrolling this loop 4 chunks deep removes the window-carry moves but measured
        // 1.5% slower on C3: kept rolled)
        for (int q0 = 0; q0 < a.Q; q0 += QC) {
            TT hv[QC];
            DT nx[QC];
#pragma unroll
            for (int u = 0; u < QC; u++) hv[u] = Hp[q0 + u];
#pragma unroll
            for (int u = 0; u < QC; u++) nx[u] = Xj[u % K][1 + (q0 + u) / K];   // row l*K + K + q0 + u
#pragma unroll
            for (int u = 0; u < QC; u++) {
#pragma unroll
                for (int i = 0; i < K; i++) mac(acc[i], w[(i + u) % K], hv[u]);
                w[u % K] = nx[u];
            }
        }
    }

    if constexpr (QUAD) {
        // FM quadrature (demod/quadrature.h:41-56): out = arg(y[m] * conj(y[m-1])) / dev
        lastY[l] = acc[K - 1];
        const float2 din0 = a.din[0];                 // y[-1] of the stream: carried from the last call
        __syncthreads();
        float* out = reinterpret_cast<float*>(a.out);
        const float2 left = lastY[l > 0 ? l - 1 : 0];
#pragma unroll
        for (int i = 0; i < K; i++) {
            const int m = mFirst + l * K + i;
            if (m >= 0 && m >= tile * a.TMS && m < a.M) {
                float2 prev = (i > 0) ? acc[i > 0 ? i - 1 : 0] : left;
                if (m == 0) prev = din0;
                const float2 y = acc[i];
                const float br = prev.x, bi = -prev.y;
                const float re = (y.x * br) - (y.y * bi);
                const float im = (y.y * br) + (y.x * bi);
                out[m] = quad_atan2f(im, re) * a.invDev;
                if (m == a.M - 1) a.dinNext[0] = y;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < K; i++) {
            const int m = mFirst + l * K + i;
            if (m < a.M && m < (tile + 1) * a.TMS) {
                if constexpr (STEREO) {
                    reinterpret_cast<float2*>(a.out)[m] = make_float2(acc[i], acc[i]);   // LRToStereo(l = r)
                } else {
                    reinterpret_cast<DT*>(a.out)[m] = acc[i];
                }
            }
        }
    }
}

}  // namespace sdrgpu
