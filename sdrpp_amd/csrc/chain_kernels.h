// The small kernels of the channel chain (blocks.hip): the per-call NCO table, the history carry of a
// call without outputs, the frequency xlator, the FM quadrature, BroadcastFM mono in one launch (short
// and big calls), the polyphase resampler and the ingest converters.
#pragma once
#include "sdrgpu_internal.h"
#include "fir_rows.h"

namespace sdrgpu {

// ------------------------------------------------------------------- helpers
__global__ void nco_hi_kernel(float2* __restrict__ phi, int n, double theta0, double w) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    phi[j] = nco_phi(theta0, w, j);
}

// the history carry (fir.h:80) of a call that yields no output; with outputs, the FIR launch's own last
// workgroup carries it (fir_rows.h fir_hist_block)
template <typename DT, bool XL>
__global__ void fir_hist_kernel(const DT* __restrict__ hist, const DT* __restrict__ in, DT* __restrict__ next, int H,
                                int count, const float2* __restrict__ phi, const float2* __restrict__ plo) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= H) return;
    const long long b = (long long)count + k;
    DT v;
    if (b < H) {
        v = hist[b];
    } else {
        const long long i = b - H;
        v = in[i];
        if constexpr (XL) v = cmulf(v, nco_tab(phi, plo, i));
    }
    next[k] = v;
}

// --------------------------------------------------------------- xlator
__global__ void xlator_kernel(const float2* __restrict__ in, float2* __restrict__ out, long long n,
                              const float2* __restrict__ phi, const float2* __restrict__ plo) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = cmulf(in[i], nco_tab(phi, plo, i));
}

// ----------------------------------------------------------- quadrature
// (quad_value: quad_value.h)
__global__ void quad_kernel(const float2* __restrict__ in, float* __restrict__ out, int n, const float2* __restrict__ din,
                            float2* __restrict__ dinNext, float invDev) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 y = in[i];
    out[i] = quad_value(y, i ? in[i - 1] : din[0], invDev);
    if (i == n - 1) dinNext[0] = y;
}

// BroadcastFM mono for short calls (a reference block: 307,200 / 256 = 1,200 samples at
// 240 kS/s): the quadrature and the audio FIR (+ LRToStereo) in one launch instead of two
// 5-7 us ones. Workgroup b computes outputs [256 b, 256 b + 256) from the quadrature values of
// its window of [hist || quad(in)] (halo recomputed), with the FIR's tap order and fmaf chain
// (fir_kernel at D = 1), so the outputs are bit-identical to the two-launch path; the last
// workgroup writes the next call's FIR history and y[-1].
constexpr int WFM_TM = 256;
__global__ __launch_bounds__(WFM_TM) void wfm_short_kernel(
    const float2* __restrict__ in, int count, const float2* __restrict__ din, float2* __restrict__ dinNext,
    const float* __restrict__ hist, float* __restrict__ histNext, const float* __restrict__ taps, int Q, int H,
    float invDev, float2* __restrict__ out) {
    extern __shared__ float X[];
    const int tid = threadIdx.x;
    auto qv = [&](long long b) -> float {   // [hist || quad(in)][b], zero past the end
        if (b < H) return hist[b];
        const long long i = b - H;
        if (i >= count) return 0.0f;
        return quad_value(in[i], i ? in[i - 1] : din[0], invDev);
    };
    if (blockIdx.x == gridDim.x - 1) {
        for (int k = tid; k < H; k += WFM_TM) histNext[k] = qv((long long)count + k);
        if (tid == 0) dinNext[0] = in[count - 1];
        return;
    }
    const int m0 = blockIdx.x * WFM_TM;
    for (int j = tid; j < WFM_TM + Q; j += WFM_TM) X[j] = qv((long long)m0 + j);
    __syncthreads();
    const int m = m0 + tid;
    if (m >= count) return;
    float acc = 0.0f;
    for (int q = 0; q < Q; q++) acc = fmaf(X[tid + q], taps[q], acc);
    out[m] = make_float2(acc, acc);
}

// BroadcastFM mono for big calls (C5: 1,048,576 samples at 240 kS/s per step): the same fused form
// with K = 4 outputs per thread (1,024 per workgroup). The quadrature values of the window go to LDS in
// fir_tail's row layout (element e at row e mod K, column e / K: a thread's K-output register window
// reads consecutive columns, conflict-free), rows r and r + K/2 interleaved as float pairs, so the
// thread's outputs i and i + K / 2 run as one packed fp32 FMA (v_pk_fma_f32; each lane is the fmaf of the
// scalar chain, same bits) over the padded taps in tap order (fir_kernel at D = 1): the window pair of
// outputs (i, i + K/2) at tap u is rows ((i + u) mod K, (i + u + K/2) mod K), one stored pair, swapped
// (op_sel) when (i + u) mod K >= K/2. No quadrature round trip through HBM (quad_kernel +
// fir_kernel<float, float, 4>: 5.3 + 15.6 us per C5 step, r5m; scalar chains in this kernel 15.7 us).
constexpr int WFM_BK = 4;   // outputs per thread (r6o: 14.6 vs 15.1 us per C5 step at 8, same bits)
constexpr int WFM_BNT = 256, WFM_BCH = WFM_BK * WFM_BNT;
__global__ __launch_bounds__(WFM_BNT) void wfm_big_kernel(
    const float2* __restrict__ in, int count, const float2* __restrict__ din, float2* __restrict__ dinNext,
    const float* __restrict__ hist, float* __restrict__ histNext, const float* __restrict__ taps, int Q, int H,
    float invDev, float2* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float X[];
    constexpr int K = WFM_BK;
    const int tid = threadIdx.x;
    auto qv = [&](long long b) -> float {   // [hist || quad(in)][b], zero past the end
        if (b < H) return hist[b];
        const long long i = b - H;
        if (i >= count) return 0.0f;
        return quad_value(in[i], i ? in[i - 1] : din[0], invDev);
    };
    if (blockIdx.x == gridDim.x - 1) {
        for (int k = tid; k < H; k += WFM_BNT) histNext[k] = qv((long long)count + k);
        if (tid == 0) dinNext[0] = in[count - 1];
        return;
    }
    const long long m0 = (long long)blockIdx.x * WFM_BCH;
    const int RSK = WFM_BNT + Q / K + 2;   // columns per row (Q is a multiple of 8, <= 256: host-checked)
    float* T = X + K * RSK;                // the taps
    const f2v* P = reinterpret_cast<const f2v*>(X);   // P[r * RSK + c] = (row r, row r + K/2) at column c, r < K/2
    auto at = [&](int j) { return 2 * ((j % (K / 2)) * RSK + j / K) + (j / (K / 2)) % 2; };   // float index of element j
    for (int q = tid; q < Q; q += WFM_BNT) T[q] = taps[q];
    // the window [m0, m0 + K RSK) of [hist || quad(in)]: interior workgroups issue all their sample
    // loads at once (one memory round trip), the first and last take the element-wise path
    constexpr int NF = (K * (WFM_BNT + 256 / K + 2) + WFM_BNT - 1) / WFM_BNT;
    if (m0 >= H + 1 && m0 + K * RSK - H <= count) {
        float2 y[NF], yp[NF];
        const float2* src = in + (m0 - H);
#pragma unroll
        for (int k = 0; k < NF; k++) {
            const int j = tid + k * WFM_BNT;
            const int jj = j < K * RSK ? j : 0;
            y[k] = src[jj];
            yp[k] = src[jj - 1];
        }
#pragma unroll
        for (int k = 0; k < NF; k++) {
            const int j = tid + k * WFM_BNT;
            if (j < K * RSK) X[at(j)] = quad_value(y[k], yp[k], invDev);
        }
    } else {
        for (int j = tid; j < K * RSK; j += WFM_BNT) X[at(j)] = qv(m0 + j);
    }
    __syncthreads();
    f2v acc[K / 2], w[K / 2];   // acc[i] = outputs (i, i + K/2); w[r] = window rows (r, r + K/2)
#pragma unroll
    for (int i = 0; i < K / 2; i++) {
        acc[i] = f2v{0.f, 0.f};
        w[i] = P[i * RSK + tid];
    }
    for (int q0 = 0; q0 < Q; q0 += K) {
        float hv[K];
        f2v nx[K / 2];
#pragma unroll
        for (int u = 0; u < K; u++) hv[u] = T[q0 + u];   // (LDS broadcasts)
#pragma unroll
        for (int r = 0; r < K / 2; r++) nx[r] = P[r * RSK + tid + 1 + q0 / K];
#pragma unroll
        for (int u = 0; u < K; u++) {
#pragma unroll
            for (int i = 0; i < K / 2; i++) {
                const int r = (i + u) % K;
                const f2v x = r < K / 2 ? w[r] : __builtin_shufflevector(w[r - K / 2], w[r - K / 2], 1, 0);
                acc[i] = __builtin_elementwise_fma(x, f2v{hv[u], hv[u]}, acc[i]);
            }
            if (u < K / 2) w[u].x = nx[u].x;   // row u slides to the next column
            else w[u - K / 2].y = nx[u - K / 2].y;
        }
    }
    float a[K];
#pragma unroll
    for (int i = 0; i < K / 2; i++) {
        a[i] = acc[i].x;
        a[i + K / 2] = acc[i].y;
    }
    const long long m = m0 + (long long)tid * K;
    if (m + K <= count) {
        float4* o = reinterpret_cast<float4*>(out + m);   // (out: 8-byte stereo frames; 16-B aligned pairs)
        if (((uintptr_t)out & 15) == 0) {
#pragma unroll
            for (int i = 0; i < K; i += 2) o[i / 2] = make_float4(a[i], a[i], a[i + 1], a[i + 1]);
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < K; i++)
        if (m + i < count) out[m + i] = make_float2(a[i], a[i]);
}

// ------------------------------------------------ polyphase resampler
// multirate/polyphase_resampler.h:69-99 in closed form: with pos = offset*interp + phase,
// output m uses pos_m = pos0 + m*decim -> (offset_m, phase_m) = divmod(pos_m, interp).
template <typename DT>
__global__ void poly_kernel(const DT* __restrict__ hist, const DT* __restrict__ in, const float* __restrict__ bank,
                            DT* __restrict__ out, int H, int tpp, int interp, int decim, long long pos0, int M) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const long long pos = pos0 + (long long)m * decim;
    const long long off = pos / interp;
    const int ph = (int)(pos % interp);
    const float* hb = bank + (size_t)ph * tpp;
    DT acc = zero_of<DT>();
    for (int j = 0; j < tpp; j++) {
        const long long b = off + j;
        const DT x = b < H ? hist[b] : in[b - H];
        mac(acc, x, hb[j]);
    }
    out[m] = acc;
}

// ------------------------------------------------------------ converters
__device__ __forceinline__ float convert_one(int kind, const void* __restrict__ in, long long i) {
    switch (kind) {
    case SDRGPU_CONV_U8: return (((const uint8_t*)in)[i] - 128 + 0.5f) / (128.0f - 0.5f);
    case SDRGPU_CONV_I16: return (((const int16_t*)in)[i] + 0.5f) / (32768.0f - 0.5f);
    case SDRGPU_CONV_I24: {
        const uint8_t* p = (const uint8_t*)in + 3 * i;
        int32_t v = (int32_t)((uint32_t)(p[0] | (p[1] << 8) | (p[2] << 16)) << 8) >> 8;
        return (v + 0.5f) / (8388608.0f - 0.5f);
    }
    case SDRGPU_CONV_I32: return (float)((((const int32_t*)in)[i] + 0.5) / (2147483648.0 - 0.5));
    case SDRGPU_CONV_F64: return (float)((const double*)in)[i];
    case SDRGPU_CONV_I8: return ((float)((const int8_t*)in)[i]) * (float)(1.0 / 128.0f);
    default: return ((const float*)in)[i];   // SDRGPU_CONV_F32: IEEE float samples as they are
    }
}
__global__ void convert_kernel(int kind, const void* __restrict__ in, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = convert_one(kind, in, i);
}
// one-channel WAV (file_source worker_1ch, main.cpp:294-430): I = Q = the converted sample
__global__ void convert_mono_kernel(int kind, const void* __restrict__ in, long long n, float2* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = convert_one(kind, in, i);
    out[i] = make_float2(v, v);
}

}  // namespace sdrgpu
