// The matrix-core FIR kernels of the channel chain (blocks.hip FirBlock): complex data x real taps at
// power-of-two decimations -- fir_mfma_kernel (C3: D <= 8, 16..32 taps per phase) and its phase-split
// variant fir_mfma_ps_kernel (D = 4..32, fewer taps per phase).
#pragma once
#include "fir_rows.h"

namespace sdrgpu {

// ------------------------------------------------ MFMA FIR (complex data x real taps)
// With Qp = ceil(ntaps / D) taps per phase (C3: 256 taps / 8 = 32), each phase's correlation
//   y_p[m] = sum_q g_p[q] u_p[m + q],   u_p[n] = span[n D + p],   g_p[q] = h[q D + p]
// is a Toeplitz product and runs on the f32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32
// FMA chains at the vector-FMA peak, one VGPR per operand, no VALU issue):
//   Y[i][j] += sum_k A[i][k] B[k][j],   A[i][k] = u_p[o + 16 i + k],   B[k][j] = g_p[k - j]
// (zero outside [0, Qp)), so the 16 x 16 accumulator holds outputs o + 16 i + j and k runs over
// [0, 16 + Qp - 1) in steps of 4 (1.47x the essential MACs at Qp = 32). Re and im are two
// accumulators sharing B. A wave owns 256 consecutive outputs, a workgroup MF_TM = 1024.
// LDS: the span phase-major with one pad row per 16 (X[p][r + r / 16]: the 16 rows of one A
// load fall in distinct banks), and B as gz[p][t] = g_p[t - 15], t < 64 (host-built).
typedef float f32x4_t __attribute__((ext_vector_type(4)));
constexpr int MF_KS = 12;                   // k steps of 4: k < 48 >= 16 + Qp - 1 for Qp <= 32
constexpr int MF_GZ = 64;                   // gz entries per phase
constexpr int mf_rows(int nw) { return 256 * nw + 4 * MF_KS; }   // span rows per phase

// HALF (round 4): only half of the D phases' span rows are in LDS at a time -- a thread's span
// loads all belong to one phase (NT % D == 0), so the threads of the upper phases keep theirs in
// registers while the MFMAs run over the lower phases, then store them into the same LDS. Half the
// LDS per workgroup: four workgroups (16 waves) per CU instead of two, the same MFMA chains in the
// same order (bit-identical outputs).
// DC (round 4): the decimation as a compile-time constant (0: a.D at run time). C3's D = 8 then has a
// constant span, so the PF load / store slots need no range guards (only the last is partial) and the
// LDS indices fold: the SQ counters showed the SIMD ~90% busy with MFMA + VALU issue (no co-issue on
// the f32 matrix path), so every VALU instruction saved is kernel time.
template <int NW, bool XL, bool QUAD, bool HALF = false, int DC = 0>   // NW waves per workgroup, 256 outputs each
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(HALF ? 4 : 1))) void fir_mfma_kernel(FirArgs a) {
    if (fir_hist_block<float2, XL>(a)) return;
    constexpr int NT = 64 * NW, MF_TM = 256 * NW, MF_ROWS = mf_rows(NW);
    constexpr int PF = (MF_ROWS * 8 + NT - 1) / NT;    // load slots per thread for D <= 8
    constexpr int QOFF = QUAD ? 1 : 0;
    constexpr int NH = HALF ? 2 : 1;                   // phase halves through LDS
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2* X = reinterpret_cast<float2*>(smem);
    float* gz = reinterpret_cast<float*>(smem + a.tapsLdsOff);
    const int tid = threadIdx.x, tile = blockIdx.x;
    // D a power of two dividing NT (host-checked); RSP = MF_ROWS + MF_ROWS / 16 + 1 (run_mfma_nw)
    const int D = DC ? DC : a.D, RSP = DC ? MF_ROWS + MF_ROWS / 16 + 1 : a.RSP;
    const int dsh = DC ? __builtin_ctz((unsigned)(DC ? DC : 1)) : a.dshift;
    const int DH = D / NH;                            // phases in LDS at a time
    {
        const float* __restrict__ g = reinterpret_cast<const float*>(a.taps);
        for (int i = tid; i < D * MF_GZ; i += NT) gz[i] = g[i];
    }
    auto lds_index = [&](int sx) {   // (HALF: the phase's slot within its half)
        const int r = sx >> dsh, p = sx & (D - 1);
        return (p % DH) * RSP + r + (r >> 4);
    };
    const int mFirst = tile * a.TMS - QOFF;
    const long long b0 = (long long)a.offset0 + (long long)mFirst * D;
    const int span = MF_ROWS * D;
    const bool interior = (b0 >= a.H) && (b0 + span <= (long long)a.H + a.count);
    float2 pf[PF];
    if (interior) {
        // XL: the NCO phase of slot 0 is computed before the PF loads are issued (its sincos
        // temporaries would otherwise be live next to the 2 x PF loaded registers)
        float2 ph0 = make_float2(1.f, 0.f);
        if constexpr (XL) {
            ph0 = nco_at(a, b0 - a.H + tid);
            __builtin_amdgcn_sched_barrier(0);
        }
        // one wave-uniform buffer resource and ONE per-lane offset for all PF loads, the slot step
        // in the scalar offset (no per-slot 64-bit address registers; interior: no range check needed)
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float2*>(reinterpret_cast<const float2*>(a.in) + (b0 - a.H)), (short)0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int u = 0; u < PF; u++) {
            const int sx = tid + u * NT;
            if (sx < span) pf[u] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, tid * 8, u * NT * 8, 0));
        }
        if constexpr (XL) {
            // the wave-uniform step table through the constant address space: scalar loads, so
            // the 2 x PF step values do not take VGPRs next to the PF loaded samples
            const __attribute__((address_space(4))) float* S = (const __attribute__((address_space(4))) float*)a.nstep;
#pragma unroll
            for (int u = 0; u < PF; u++) pf[u] = xlate_slot(pf[u], ph0, make_float2(S[2 * u], S[2 * u + 1]));
        }
    }
    const int lane = tid & 63, o = (tid >> 6) * 256;
    const int i = lane & 15, kk = lane >> 4;   // A row i / B column j = i, k offset kk
    f32x4_t cre = {0.f, 0.f, 0.f, 0.f}, cim = {0.f, 0.f, 0.f, 0.f};
    const int myHalf = (tid & (D - 1)) / DH;   // the phase half this thread's span slots belong to
    auto mfma_half = [&](int h) {
        for (int p = h * DH; p < (h + 1) * DH; p++) {
            const float2* Xp = X + (p - h * DH) * RSP;
            const float* gp = gz + p * MF_GZ + 15 - i + kk;   // B[k0 + kk][i] = g_p[k0 + kk - i]
            const int r0 = o + 16 * i + kk;
#pragma unroll
            for (int s = 0; s < MF_KS; s++) {
                const int r = r0 + 4 * s;
                const float2 xa = Xp[r + (r >> 4)];
                const float bb = gp[4 * s];
                cre = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.x, bb, cre, 0, 0, 0);
                cim = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.y, bb, cim, 0, 0, 0);
                // HALF: the upper half's PF samples are still live through these MFMAs; fence
                // the LDS loads in groups of 4 k steps so they are not all hoisted (no spill)
                if constexpr (HALF) if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    // the interior and edge tiles run separate half loops: pf is not live across the edge path's
    // NCO fetches (one shared loop keeps it live there and spills the HALF kernel)
    if (interior) {
#pragma unroll
        for (int h = 0; h < NH; h++) {
            if (h > 0) __syncthreads();   // every MFMA read of the previous half is done
            if (myHalf == h) {
                // slot u: phase tid % D fixed, row advancing by NT / D (+ its pad rows)
                int idx = lds_index(tid);
                const int inc = (NT >> dsh) + (NT >> dsh) / 16;
#pragma unroll
                for (int u = 0; u < PF; u++) {
                    if (tid + u * NT < span) X[idx] = pf[u];
                    idx += inc;
                }
            }
            // (HALF runs only for D <= 8, where the PF slots cover the span: host-checked)
            if constexpr (!HALF)
                for (int sx = tid + PF * NT; sx < span; sx += NT) X[lds_index(sx)] = fir_fetch<float2, XL>(a, b0 + sx);
            __syncthreads();
            mfma_half(h);
        }
    } else {
        for (int h = 0; h < NH; h++) {
            if (h > 0) __syncthreads();
            for (int sx = tid; sx < span; sx += NT)
                if (((sx & (D - 1)) / DH) == h) X[lds_index(sx)] = fir_fetch<float2, XL>(a, b0 + sx);
            __syncthreads();
            mfma_half(h);
        }
    }
    // accumulator element e of this lane: row (lane >> 4) * 4 + e, column lane & 15
    if constexpr (QUAD) {
        // FM quadrature (demod/quadrature.h:41-56) on the tile's outputs staged in LDS (the span
        // is dead once every wave has passed the barrier); output 0 of the tile only supplies y[m-1]
        float2* Y = X;
        const float2 din0 = a.din[0];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; e++) Y[o + 16 * (kk * 4 + e) + i] = make_float2(cre[e], cim[e]);
        __syncthreads();
        float* out = reinterpret_cast<float*>(a.out);
#pragma unroll
        for (int e = 0; e < MF_TM / NT; e++) {
            const int ml = tid + e * NT;
            const int m = mFirst + ml;
            if (ml >= QOFF && m >= 0 && m < a.M) {
                const float2 y = Y[ml];
                const float2 prev = (m == 0) ? din0 : Y[ml - 1];
                const float br = prev.x, bi = -prev.y;
                const float re = (y.x * br) - (y.y * bi);
                const float im = (y.y * br) + (y.x * bi);
                out[m] = quad_atan2f(im, re) * a.invDev;
                if (m == a.M - 1) a.dinNext[0] = y;
            }
        }
    } else {
        float2* out = reinterpret_cast<float2*>(a.out);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int m = mFirst + o + 16 * (kk * 4 + e) + i;
            if (m < a.M && m < (tile + 1) * a.TMS) out[m] = make_float2(cre[e], cim[e]);
        }
    }
}

// Phase-split variant for larger decimations (VFO stage 1: D = 32, 143 taps -> Qp = 5): a tile
// is 256 outputs, the four waves split the D phases (wave w takes p = w, w + 4, ...), each
// accumulating the whole 16 x 16 output block over its phases with k < 4 * ks (ks = ceil((15 + Qp)
// / 4) steps), and the four partial blocks are summed through LDS. Small tiles keep the span in
// LDS for D up to 32 (75 KB at D = 32, 2 workgroups per CU) and for D = 8 let 7 share a CU.
template <bool XL, bool QUAD>
__global__ __launch_bounds__(256) void fir_mfma_ps_kernel(FirArgs a) {
    if (fir_hist_block<float2, XL>(a)) return;
    constexpr int NT = 256, TM = 256, PF = 36, QOFF = QUAD ? 1 : 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2* X = reinterpret_cast<float2*>(smem);
    float* gz = reinterpret_cast<float*>(smem + a.tapsLdsOff);
    const int tid = threadIdx.x, tile = blockIdx.x;
    const int D = a.D, RSP = a.RSP, dsh = a.dshift, ks = a.Q;   // a.Q carries ks here
    {
        const float* __restrict__ g = reinterpret_cast<const float*>(a.taps);
        for (int i = tid; i < D * a.gzs; i += NT) gz[i] = g[i];
    }
    auto lds_index = [&](int sx) {
        const int r = sx >> dsh, p = sx & (D - 1);
        return p * RSP + r + (r >> 4);
    };
    const int rows = TM + 4 * ks;
    const int span = rows * D;
    const int mFirst = tile * a.TMS - QOFF;
    const long long b0 = (long long)a.offset0 + (long long)mFirst * D;
    const bool interior = (b0 >= a.H) && (b0 + span <= (long long)a.H + a.count);
    int sxRest = tid;
    if (interior) {
        const float2* __restrict__ src = reinterpret_cast<const float2*>(a.in) + (b0 - a.H);
        float2 pf[PF];
#pragma unroll
        for (int u = 0; u < PF; u++) {
            const int sx = tid + u * NT;
            if (sx < span) pf[u] = src[sx];
        }
        if constexpr (XL) {
            const float2 ph0 = nco_at(a, b0 - a.H + tid);
            const float2* __restrict__ S = a.nstep;
#pragma unroll
            for (int u = 0; u < PF; u++) pf[u] = xlate_slot(pf[u], ph0, S[u]);
        }
#pragma unroll
        for (int u = 0; u < PF; u++) {
            const int sx = tid + u * NT;
            if (sx < span) X[lds_index(sx)] = pf[u];
        }
        sxRest = tid + PF * NT;
    }
    for (int sx = sxRest; sx < span; sx += NT) X[lds_index(sx)] = fir_fetch<float2, XL>(a, b0 + sx);
    __syncthreads();

    const int lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, kk = lane >> 4;   // A row i / B column j = i, k offset kk
    f32x4_t cre = {0.f, 0.f, 0.f, 0.f}, cim = {0.f, 0.f, 0.f, 0.f};
    for (int p = w; p < D; p += 4) {
        const float2* Xp = X + p * RSP;
        const float* gp = gz + p * a.gzs + 15 - i + kk;   // B[k0 + kk][i] = g_p[k0 + kk - i]
        const int r0 = 16 * i + kk;
#pragma unroll
        for (int s = 0; s < MF_KS; s++) {   // unrolled so the operand reads are issued ahead
            if (s < ks) {
                const int r = r0 + 4 * s;
                const float2 xa = Xp[r + (r >> 4)];
                const float bb = gp[4 * s];
                cre = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.x, bb, cre, 0, 0, 0);
                cim = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.y, bb, cim, 0, 0, 0);
            }
        }
    }
    // partial blocks of the four waves -> LDS (the span is dead after the barrier), summed per output
    float2* P = X;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; e++) P[w * TM + 16 * (kk * 4 + e) + i] = make_float2(cre[e], cim[e]);
    __syncthreads();
    auto ysum = [&](int ml) {
        const float2 q0 = P[ml], q1 = P[TM + ml], q2 = P[2 * TM + ml], q3 = P[3 * TM + ml];
        return make_float2((q0.x + q1.x) + (q2.x + q3.x), (q0.y + q1.y) + (q2.y + q3.y));
    };
    const int ml = tid, m = mFirst + ml;
    if constexpr (QUAD) {
        if (ml >= QOFF && m >= 0 && m < a.M) {
            const float2 y = ysum(ml);
            const float2 prev = (m == 0) ? a.din[0] : ysum(ml - 1);
            const float br = prev.x, bi = -prev.y;
            const float re = (y.x * br) - (y.y * bi);
            const float im = (y.y * br) + (y.x * bi);
            reinterpret_cast<float*>(a.out)[m] = quad_atan2f(im, re) * a.invDev;
            if (m == a.M - 1) a.dinNext[0] = y;
        }
    } else {
        if (m < a.M && m < (tile + 1) * a.TMS) reinterpret_cast<float2*>(a.out)[m] = ysum(ml);
    }
}

}  // namespace sdrgpu
