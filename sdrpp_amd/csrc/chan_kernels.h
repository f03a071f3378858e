// Device code of channelizer.hip (BASELINE config C4): the two-branch polyphase kernel and the
// DFT-as-GEMM form of its per-frame transform. The maths is in channelizer.hip's header.
//
// Kernel layout (chan2_kernel): L / 2 threads, each lane owns the two branches r and r + L/2, 16 frames
// per batch. A lane keeps, per branch, a 16-deep circular window of the branch's samples in registers
// and re-reads its Q taps per batch (from L2: not live across the FFT); each batch loads one new
// sample per frame and branch (coalesced: consecutive r), forms the 2 x 16 branch outputs into the
// batch's 16 LDS sequences (rotated by `rot`), then the workgroup runs the 16 M-point Stockham FFTs in
// LDS in two rounds (a lane plays two FFT roles in turn, sequences sF and sF + 8) and stores the
// channel vectors, out[m][k]. Two branches per lane because one branch per lane (L threads) needs ~180
// VGPRs and spills at 1024 threads (128-VGPR cap), while L / 2 threads have a 256-VGPR cap: 1.17 vs
// 1.63 ms per 2^28 samples on one box. The next batch's samples are prefetched across the FFTs as far
// as the registers allow (CHAN_PF2).
#pragma once
#include "sdrgpu_internal.h"
#include "fft_stages.h"
#include "wave_lds.h"

namespace sdrgpu {

constexpr int CHAN_Q = 16;   // taps per branch (prototype padded to Q*M)
// FFT form: the next batch's 16 samples of the first branch are loaded while this batch's FFTs run, and
// the second branch's first CHAN_PF2 frames as well (204 VGPRs; all 16 frames: 82 VGPRs spilled; no
// second-branch prefetch is CHAN_PF2 = 0): C4 1.158 (no prefetch) -> 1.074 (first branch) -> 1.064 ms
// (+ 8 frames), 3 interleaved runs, r4z. Not with GEMM, whose DFT already holds 236 VGPRs.
constexpr bool CHAN_PF = true;
constexpr int CHAN_PF2 = 8;
// FFT form: channel rows are written once, so they leave through streaming (nontemporal) stores
constexpr bool CHAN_NT = true;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The M = 1024 DFT of the 16 branch vectors of a batch as dense matrix products on the f32
// matrix cores (the "filterbank cast as batched MFMA GEMM" form of BASELINE C4). With
// c = 32 a + b and k = k1 + 32 k2, W_1024^(kc) = W_32^(k1 a) W_1024^(k1 b) W_32^(k2 b), so per
// frame (viewed as the 32 x 32 matrix X[a][b] = v[32 a + b]):
//   Z = F X  (F[k1][a] = W_32^(k1 a)),  Z'[k1][b] = Z[k1][b] W_1024^(k1 b),  Y = Z' F  (F symmetric),
// and Y[k1][k2] is channel k1 + 32 k2: two complex 32 x 32 x 32 products = 2 x 128
// v_mfma_f32_16x16x4_f32 per frame (512 flop per sample against the FFT's ~50). Wave w of the
// 8 owns frames w and w + 8 of the batch: all its LDS traffic stays inside its own sequences,
// so the stages need no workgroup barrier. MFMA operand layout (as fir_mfma_kernel): A[i][k]
// from lane (i = lane & 15, k = lane >> 4), B[k][j] from lane (j = lane & 15, k = lane >> 4),
// accumulator e of a lane = D[4 (lane >> 4) + e][lane & 15]. The W_32 operand of lane (i, kk)
// at k-step s of block x is W_32^((16 x + i)(4 s + kk)) in both products. Every write phase is closed
// by wave_lds_handoff (wave_lds.h).
template <int L>
__device__ __forceinline__ void chan_dft_gemm(float2* lds, const float2* twl, int tid, int mb, int m1, float2* __restrict__ out) {
    static_assert(L == 1024, "DFT-GEMM channelizer: 1024 = 32 x 32");
    constexpr int LS = Lds<L>::LS;
    const int lane = tid & 63, wv = tid >> 6;
    const int i = lane & 15, kk = lane >> 4;
    // W_32^n = W_1024^(32 n), read from the staged twiddles at each k-step (as registers the 16
    // values per lane push the kernel past 256 VGPRs)
    auto Wv = [&](int x, int s) { return twl[32 * (((16 * x + i) * (4 * s + kk)) & 31)]; };
#pragma unroll 1
    for (int fr = 0; fr < 2; fr++) {
        const int sF = wv + 8 * fr;
        float2* X = lds + sF * LS;
        f32x4 ar[2][2], ai[2][2];   // [row block][column block]
#pragma unroll
        for (int x = 0; x < 2; x++)
#pragma unroll
            for (int y = 0; y < 2; y++) ar[x][y] = ai[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
        // Z = F X: A = F (rows k1 = 16 bi + i), B = X (k = a = 4 s + kk, columns b = 16 bj + i)
#pragma unroll
        for (int s = 0; s < 8; s++)
#pragma unroll
            for (int bj = 0; bj < 2; bj++) {
                const float2 xb = X[pad16(32 * (4 * s + kk) + 16 * bj + i)];
#pragma unroll
                for (int bi = 0; bi < 2; bi++) {
                    const float2 w = Wv(bi, s);
                    ar[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, xb.x, ar[bi][bj], 0, 0, 0);
                    ar[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(-w.y, xb.y, ar[bi][bj], 0, 0, 0);
                    ai[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, xb.y, ai[bi][bj], 0, 0, 0);
                    ai[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, xb.x, ai[bi][bj], 0, 0, 0);
                }
            }
        // Z'[k1][b] = Z[k1][b] W_1024^(k1 b) (k1 b < 1024), written over X[k1][b] once every lane
        // of this wave has read its operands of X above
        wave_lds_handoff();
#pragma unroll
        for (int bi = 0; bi < 2; bi++)
#pragma unroll
            for (int bj = 0; bj < 2; bj++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int k1 = 16 * bi + 4 * kk + e, b = 16 * bj + i;
                    X[pad16(32 * k1 + b)] = cmul(make_float2(ar[bi][bj][e], ai[bi][bj][e]), twl[k1 * b]);
                }
#pragma unroll
        for (int x = 0; x < 2; x++)
#pragma unroll
            for (int y = 0; y < 2; y++) ar[x][y] = ai[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
        wave_lds_handoff();   // Z' stored by other lanes, read below as A operands
        // Y = Z' F: A = Z' (rows k1 = 16 bi + i, k = b = 4 s + kk), B = F (columns k2 = 16 bj + i)
#pragma unroll
        for (int s = 0; s < 8; s++) {
            float2 za[2];
#pragma unroll
            for (int bi = 0; bi < 2; bi++) za[bi] = X[pad16(32 * (16 * bi + i) + 4 * s + kk)];
#pragma unroll
            for (int bi = 0; bi < 2; bi++)
#pragma unroll
                for (int bj = 0; bj < 2; bj++) {
                    const float2 g = Wv(bj, s);
                    ar[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(za[bi].x, g.x, ar[bi][bj], 0, 0, 0);
                    ar[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(-za[bi].y, g.y, ar[bi][bj], 0, 0, 0);
                    ai[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(za[bi].x, g.y, ai[bi][bj], 0, 0, 0);
                    ai[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(za[bi].y, g.x, ai[bi][bj], 0, 0, 0);
                }
        }
        // channel k = k1 + 32 k2 into the sequence (natural order), then one coalesced row store
        wave_lds_handoff();   // every lane's Z' reads done before the sequence is overwritten
#pragma unroll
        for (int bi = 0; bi < 2; bi++)
#pragma unroll
            for (int bj = 0; bj < 2; bj++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int k1 = 16 * bi + 4 * kk + e, k2 = 16 * bj + i;
                    X[pad16(k1 + 32 * k2)] = make_float2(ar[bi][bj][e], ai[bi][bj][e]);
                }
        wave_lds_handoff();   // channel vector stored by other lanes, read for the row store
        const int m = mb + sF;
        if (m < m1) {
            float2* o = out + (long long)m * L;
#pragma unroll
            for (int q = 0; q < L / 64; q++) o[lane + 64 * q] = X[pad16(lane + 64 * q)];
        }
        wave_lds_handoff();   // row store's reads done before the next frame's sequence is used
    }
}

// Two branches per thread (L/2 threads), layout above. GEMM: the per-frame DFT runs as chan_dft_gemm
// (matrix cores) instead of the LDS FFT.
template <int L, bool GEMM = false>
__global__ __launch_bounds__(L / 2) void chan2_kernel(const float2* __restrict__ hist, const float2* __restrict__ in, int H,
                                                      int count, const float* __restrict__ taps, long long offset0,
                                                      int rot, int frames, int fpw, const float2* __restrict__ tw,
                                                      float2* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    constexpr int Q = CHAN_Q, T = L / 16, LS = Lds<L>::LS, NT = L / 2;
    float2* twl = lds + 16 * LS;
    twl[threadIdx.x] = tw[threadIdx.x];
    twl[threadIdx.x + NT] = tw[threadIdx.x + NT];
    float2* tw16 = twl + L;   // the middle FFT stage's twiddles, bank-conflict-free (stage_lds)
    stage16_twiddles<L>(tw16, tw, threadIdx.x, NT);
    const int m0 = blockIdx.x * fpw;
    const int m1 = min(m0 + fpw, frames);
    auto fetch = [&](long long b) -> float2 {
        if (b < H) return hist[b];
        const long long i = b - H;
        return i < count ? in[i] : make_float2(0.f, 0.f);
    };
    float2 xs[2][16];
#pragma unroll
    for (int h2 = 0; h2 < 2; h2++) {
        const long long base = offset0 + threadIdx.x + h2 * NT;
#pragma unroll
        for (int q = 0; q < 15; q++) xs[h2][q] = fetch(base + (long long)(m0 + q) * L);
        xs[h2][15] = make_float2(0.f, 0.f);
    }
    // prefetch across the FFTs (CHAN_PF): the first branch's 16 frames, the second's first PF2
    constexpr bool PFK = CHAN_PF && !GEMM;
    constexpr int PF2 = PFK ? CHAN_PF2 : 0;
    float2 pf[1][16];
    float2 pf2[PF2 > 0 ? PF2 : 1];
    // The newest tap row of the batch at mb for branches h0 .. h1 - 1, 16 frames each. Interior batch (all
    // 16 rows inside `in`): per-row uniform base + the lane's r, so the 16 loads share one offset register
    // instead of 16 64-bit addresses; else element-wise through fetch.
    auto load_batch = [&](int mb, int tid, auto& dst, int h0, int h1) {
        const long long lo = offset0 + (long long)(mb + 15) * L, hi = offset0 + (long long)(mb + 31) * L + L;
        const bool inner = mb + 16 <= m1 && lo >= H && hi <= (long long)H + count;
#pragma unroll
        for (int h2 = h0; h2 < h1; h2++) {
            const int r = tid + h2 * NT;
            if (inner) {
                const float2* __restrict__ src = in + (lo - H);
#pragma unroll
                for (int f = 0; f < 16; f++) dst[h2 - h0][f] = src[(long long)f * L + r];
            } else {
                const long long base = offset0 + r;
#pragma unroll
                for (int f = 0; f < 16; f++)
                    dst[h2 - h0][f] = (mb + f < m1) ? fetch(base + (long long)(mb + f + 15) * L) : make_float2(0.f, 0.f);
            }
        }
    };
    // The same for branch 1, frames < PF2, into pf2. Kept as a second loader: every merged form tried
    // (frame count from the destination's extent; one row per call; rows sharing one interior test)
    // reordered instructions in one of the four instantiations of this kernel, which sits at 204 VGPRs
    // next to the spill cliff described above (profiles/r10/README.md).
    auto load2 = [&](int mb, int tid) {
        if constexpr (PF2 > 0) {
            const long long lo = offset0 + (long long)(mb + 15) * L, hi = offset0 + (long long)(mb + 31) * L + L;
            const bool inner = mb + 16 <= m1 && lo >= H && hi <= (long long)H + count;
            const int r = tid + NT;
            if (inner) {
                const float2* __restrict__ src = in + (lo - H);
#pragma unroll
                for (int f = 0; f < PF2; f++) pf2[f] = src[(long long)f * L + r];
            } else {
                const long long base = offset0 + r;
#pragma unroll
                for (int f = 0; f < PF2; f++) pf2[f] = (mb + f < m1) ? fetch(base + (long long)(mb + f + 15) * L) : make_float2(0.f, 0.f);
            }
        }
    };
    if constexpr (PFK) if (m0 < m1) { load_batch(m0, threadIdx.x, pf, 0, 1); load2(m0, threadIdx.x); }
    for (int mb = m0; mb < m1; mb += 16) {
        // re-materialise the lane's LDS/FFT indices per batch instead of letting the compiler hoist
        // ~50 loop-invariant addresses out of the loop (they spill)
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        float2 cur[2][16];
        if constexpr (PFK) {
#pragma unroll
            for (int f = 0; f < 16; f++) cur[0][f] = pf[0][f];
            float2 (&c1)[1][16] = *reinterpret_cast<float2 (*)[1][16]>(&cur[1]);
            load_batch(mb, tid, c1, 1, 2);
            if constexpr (PF2 > 0) {
#pragma unroll
                for (int f = 0; f < PF2; f++) cur[1][f] = pf2[f];
            }
        } else {
            load_batch(mb, tid, cur, 0, 2);
        }
#pragma unroll
        for (int h2 = 0; h2 < 2; h2++) {
            const int r = tid + h2 * NT;
            const int c = (rot + r) & (L - 1);
            float h[Q];
#pragma unroll
            for (int q = 0; q < Q; q++) h[q] = taps[q * L + r];
            const float2 (&nx)[16] = cur[h2];
#pragma unroll
            for (int f = 0; f < 16; f++) {
                xs[h2][(f + 15) & 15] = nx[f];
                float2 u = make_float2(0.f, 0.f);
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    const float2 x = xs[h2][(f + q) & 15];
                    u.x = fmaf(h[q], x.x, u.x);
                    u.y = fmaf(h[q], x.y, u.y);
                }
                lds[f * LS + pad16(c)] = u;
            }
        }
        __syncthreads();
        if constexpr (PFK) if (mb + 16 < m1) { load_batch(mb + 16, tid, pf, 0, 1); load2(mb + 16, tid); }
        if constexpr (GEMM) {
            chan_dft_gemm<L>(lds, twl, tid, mb, m1, out);
            __syncthreads();
            continue;
        }
#pragma unroll 1
        for (int half = 0; half < 2; half++) {
            const int sF = tid / T + 8 * half, tF = tid % T;
            float2 v[16];
#pragma unroll
            for (int i = 0; i < 16; i++) v[i] = lds[sF * LS + pad16s<T>(tF, i)];
            __syncthreads();
            stage_first<L>(lds + sF * LS, v, tF);
            __syncthreads();
            const int m = mb + sF;
            float2* o = out + (long long)m * L;
            stages_rest<L, (L >= 256)>(lds, twl, sF, tF, [&](int k, float2 y) {
                if (m < m1) {
                    if constexpr (CHAN_NT) {
                        typedef float f2v __attribute__((ext_vector_type(2)));
                        __builtin_nontemporal_store(f2v{y.x, y.y}, reinterpret_cast<f2v*>(o + k));
                    } else {
                        o[k] = y;
                    }
                }
            }, tw16);
            __syncthreads();
        }
    }
}

}  // namespace sdrgpu
