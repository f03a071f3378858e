// Device code of ifnr.hip: the FMIF GEMM kernel with its DPP row reductions, and the three Squelch
// kernels. The method and the layout are described in ifnr.hip's header.
#pragma once
#include "sdrgpu_internal.h"
#include "wave_lds.h"

namespace sdrgpu {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int IF_NT = 256;              // 4 waves, 256 outputs each
constexpr int IF_TM = 1024;             // outputs per workgroup
constexpr int IF_XN = IF_TM + 32;       // span: the tile + up to 31 more (n < 32)
constexpr int IF_TAB = 2 * 32 * 32 + 2 * 32;   // cr | ci | ph floats

struct FmifArgs {
    const float2* in;
    float2* out;
    const float2* hist;
    float2* histNext;
    const float* tab;
    int count, B, ntiles;
};

template <int CTRL>
__device__ __forceinline__ float dpp_row_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ int dpp_row_i(int v) {
    return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false);
}
// all-reduce over a 16-lane DPP row (row_ror:1, 2, 4, 8)
__device__ __forceinline__ float row_max(float v) {
    v = fmaxf(v, dpp_row_f<0x121>(v));
    v = fmaxf(v, dpp_row_f<0x122>(v));
    v = fmaxf(v, dpp_row_f<0x124>(v));
    return fmaxf(v, dpp_row_f<0x128>(v));
}
__device__ __forceinline__ int row_min(int v) {
    v = min(v, dpp_row_i<0x121>(v));
    v = min(v, dpp_row_i<0x122>(v));
    v = min(v, dpp_row_i<0x124>(v));
    return min(v, dpp_row_i<0x128>(v));
}

// KS k steps of 4 (n < 4 KS >= B); one bin tile for B <= 16, two above
template <int KS>
__global__ __launch_bounds__(IF_NT) void fmif_kernel(FmifArgs a) {
    constexpr int NY = KS > 4 ? 2 : 1;
    const int tid = threadIdx.x, H = a.B - 1;
    if ((int)blockIdx.x == a.ntiles) {   // next call's history: the last H of [hist || in]
        for (int k = tid; k < H; k += IF_NT) {
            const long long b = (long long)a.count + k;
            a.histNext[k] = b < H ? a.hist[b] : a.in[b - H];
        }
        return;
    }
    __shared__ float2 X[IF_XN];
    __shared__ float2 Y[IF_TM];
    const long long m0 = (long long)blockIdx.x * IF_TM;
    for (int j = tid; j < IF_XN; j += IF_NT) {
        const long long b = m0 + j;                            // index into [hist || in], 0 beyond it
        float2 v = make_float2(0.f, 0.f);
        if (b < H) v = a.hist[b];
        else if (b - H < a.count) v = a.in[b - H];
        X[j] = v;
    }
    const int lane = tid & 63, o = (tid >> 6) * 256;
    const int i = lane & 15, kk = lane >> 4;   // A row i / B column i, k offset kk
    float br[KS][NY], bi[KS][NY];
    float2 ph[NY];
    bool valid[NY];
#pragma unroll
    for (int y = 0; y < NY; y++) {
#pragma unroll
        for (int s = 0; s < KS; s++) {
            br[s][y] = a.tab[(4 * s + kk) * 32 + 16 * y + i];
            bi[s][y] = a.tab[32 * 32 + (4 * s + kk) * 32 + 16 * y + i];
        }
        ph[y] = reinterpret_cast<const float2*>(a.tab + 2 * 32 * 32)[16 * y + i];
        valid[y] = 16 * y + i < a.B;
    }
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < 16; t++) {
        const int sb = o + 16 * t;                             // 16 samples sb .. sb + 15 of the tile
        if (m0 + sb >= a.count) break;                         // (wave-uniform)
        f32x4_t are[NY], aim[NY];
#pragma unroll
        for (int y = 0; y < NY; y++) are[y] = aim[y] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; s++) {
            const float2 xa = X[sb + i + 4 * s + kk];
            const float nxi = -xa.y;
#pragma unroll
            for (int y = 0; y < NY; y++) {
                are[y] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.x, br[s][y], are[y], 0, 0, 0);
                aim[y] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.x, bi[s][y], aim[y], 0, 0, 0);
            }
#pragma unroll
            for (int y = 0; y < NY; y++) {
                are[y] = __builtin_amdgcn_mfma_f32_16x16x4f32(nxi, bi[s][y], are[y], 0, 0, 0);
                aim[y] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.y, br[s][y], aim[y], 0, 0, 0);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {                          // sample sb + 4 kk + e, bins 16 y + i
            float re = are[0][e], im = aim[0][e];
            // (fmaxf drops a NaN, so the pair order below is total and exactly one lane wins)
            float mg = valid[0] ? fmaxf(re * re + im * im, 0.f) : -1.f;
            int k = i;
            float2 p = ph[0];
            if constexpr (NY == 2) {
                const float re1 = are[1][e], im1 = aim[1][e];
                const float m1 = valid[1] ? fmaxf(re1 * re1 + im1 * im1, 0.f) : -1.f;
                if (m1 > mg) {                                 // a tie keeps the lower bin
                    mg = m1;
                    k = 16 + i;
                    re = re1;
                    im = im1;
                    p = ph[1];
                }
            }
            const float top = row_max(mg);
            const int win = row_min(mg == top ? k : 64);
            if (win == k) Y[sb + 4 * kk + e] = make_float2(re * p.x - im * p.y, re * p.y + im * p.x);
        }
    }
    wave_lds_handoff();   // Y of this wave's 256 samples, stored by other lanes
    float2* out = a.out + m0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int ml = o + lane + 64 * q;
        if (m0 + ml < a.count) out[ml] = Y[ml];
    }
}

// ------------------------------------------------------------------ Squelch
constexpr int SQ_NT = 256;
constexpr int SQ_CHUNK = 4096;   // samples per partial sum

struct SquelchState {
    int muted, cnt;
};

// fixed-order sum of the workgroup's SQ_NT values; the result in every thread
__device__ __forceinline__ float sq_tree(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = SQ_NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// volk_32fc_magnitude_32f + volk_32f_accumulator_s32f (squelch.h:35-36), one chunk per workgroup
__global__ __launch_bounds__(SQ_NT) void squelch_partial_kernel(const float2* __restrict__ in, int count, float* __restrict__ part) {
    __shared__ float red[SQ_NT];
    const long long i0 = (long long)blockIdx.x * SQ_CHUNK;
    const int n = (int)min((long long)SQ_CHUNK, count - i0);
    float sum = 0.0f;
    for (int i = threadIdx.x; i < n; i += SQ_NT) {
        const float2 v = in[i0 + i];
        sum += sqrtf(v.x * v.x + v.y * v.y);
    }
    sum = sq_tree(sum, red);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// one workgroup: the sum of the partials, then the decision (squelch.h:37-53)
__global__ __launch_bounds__(SQ_NT) void squelch_decide_kernel(const float* __restrict__ part, int nparts, int count, float L,
                                                              SquelchState* __restrict__ st) {
    __shared__ float red[SQ_NT];
    float sum = 0.0f;
    for (int i = threadIdx.x; i < nparts; i += SQ_NT) sum += part[i];
    sum = sq_tree(sum, red);
    if (threadIdx.x != 0) return;
    sum /= (float)count;
    const float level = 20.0f * log10f(sum);
    int muted = st->muted, cnt = st->cnt;
    if (muted) {
        if (level < L || cnt <= 0) cnt = 10;        // 10 calls above the level before unmute
        else if (--cnt == 0) muted = 0;
    } else if (level < (L - 1.0f)) {                // 1 dB hysteresis
        cnt = 0;
        muted = 1;
    }
    st->muted = muted;
    st->cnt = cnt;
}

__global__ __launch_bounds__(SQ_NT) void squelch_gate_kernel(const float2* __restrict__ in, float2* __restrict__ out, int count,
                                                            const SquelchState* __restrict__ st) {
    const long long i = (long long)blockIdx.x * SQ_NT + threadIdx.x;
    if (i >= count) return;
    out[i] = st->muted ? make_float2(0.f, 0.f) : in[i];   // memset / memcpy (squelch.h:55-60)
}

}  // namespace sdrgpu
