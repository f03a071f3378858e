// Spectrum device code, two-pass side: the dB epilogue (db_of), the tile loop, the single-pass,
// pass-A, paired pass-A, 1M and pass-B tiles and kernels, the merged pass-B + pass-A launch, and the
// launch that carries a VFO's first stage beside the passes (fft_vfo_kernel). Host side: fft.hip;
// the front end's per-block pair built from these tiles: fft_split.h.
// In-LDS FFT: Stockham autosort, radix-16 butterflies in registers (radix 2/4/8 for the last
// stage), one pad element per 16 so strided writes avoid bank conflicts, twiddles from an
// fp64-generated table (fft_stages.h).
#pragma once
#include "sdrgpu_internal.h"
#include "fft_stages.h"
#include "fir_rows.h"
#include "fir_tail.h"

namespace sdrgpu {

// K3, volk_32fc_s32f_power_spectrum_32f(out, X, 1.0, N): 10*log10(re^2 + im^2).
// VOLK evaluates 10 * log10f(p) in fp32, which adds about one ulp of the dB value on top of the
// FFT's own error (median 1 ulp vs the correctly rounded dB of the exact DFT). Here the exponent
// of p is split off exactly (p = m 2^e, m in [0.5, 1)), only log2(m) is taken in fp32 (absolute
// error ~1e-7), and e + log2(m) is scaled by 10 log10(2) in fp64 and rounded once: the dB row
// then carries the FFT's error only (median 0 ulp, same class as pocketfft + an exact log;
// tests/test_gpu_parity.py::test_spectrum_ulp_distribution). Three fp64 ops per bin in a
// memory-bound epilogue. p = 0 gives -inf like log10f.
__device__ __forceinline__ float db_of(float2 X) {
    const float p = X.x * X.x + X.y * X.y;
    int e;
    const float m = frexpf(p, &e);
    const double l = (double)e + (double)__builtin_amdgcn_logf(m);   // v_log_f32: log2, m normal or 0
    return (float)(3.0102999566398119521 * l);
}

// Persistent tile loop shared by the three spectrum kernels. Each workgroup walks tiles
// blockIdx.x, +gridDim.x, ...; the 16 raw loads of tile i+1 (Frag) are issued before tile i
// is transformed and stored, so HBM latency overlaps the LDS exchange, the math and the
// stores of the previous tile (one register fragment in flight per thread).
template <int L, class Frag, bool T16 = false, class Issue, class Finish, class Store>
__device__ __forceinline__ void tile_loop(float2* lds, const float2* __restrict__ tw, int tile, int ntiles, int sF, int tF,
                                          int sL, int tL, Issue&& issue, Finish&& finish, Store&& store,
                                          const float2* tw16 = nullptr) {
    // One tile per workgroup (grid = tiles). A persistent variant with a ping-pong register
    // prefetch of the next tile was measured at the same 64k throughput with a quarter of the
    // occupancy (and spills at N1 = 1024), so the simple form is kept.
    constexpr int LS = Lds<L>::LS;
    if (tile >= ntiles) return;
    Frag fr;
    issue(fr, tile);
    float2 v[16];
    finish(fr, v);
    stage_first<L>(lds + sF * LS, v, tF);
    __syncthreads();
    stages_rest<L, T16>(lds, tw, sL, tL, [&](int k, float2 y, int slot) {
        if constexpr (std::is_invocable_v<Store&, int, int, float2, int>) store(tile, k, y, slot);
        else store(tile, k, y);
    }, tw16);
}

struct FragW {   // raw input + window values for 16 samples
    float2 x[16];
    float w[16];
};
struct FragC {
    float2 x[16];
};

// ---- single pass (N <= 4096): S frames per tile -------------------------------
template <int L, int S>
__global__ __launch_bounds__(S * L / 16) void fft_single_kernel(
    const float2* __restrict__ in, long long frameStride, int frames, const float* __restrict__ win, int nz,
    const float2* __restrict__ tw, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    constexpr int T = L / 16;
    const int tid = threadIdx.x;
    const int s = tid / T, t = tid % T;           // frame-contiguous mapping for load and store
    const int ntiles = (frames + S - 1) / S;
    tile_loop<L, FragW>(
        lds, tw, blockIdx.x, ntiles, s, t, s, t,
        [&](FragW& fr, int tile) {
            const int f = min(tile * S + s, frames - 1);
            const float2* x = in + (long long)f * frameStride;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int n = t + r * T;
                const int nc = n < nz ? n : nz - 1;
                fr.x[r] = x[nc];
                fr.w[r] = n < nz ? win[nc] : 0.0f;
            }
        },
        [&](const FragW& fr, float2 (&v)[16]) {
#pragma unroll
            for (int r = 0; r < 16; r++) v[r] = make_float2(fr.x[r].x * fr.w[r], fr.x[r].y * fr.w[r]);
        },
        [&](int tile, int k, float2 y) {
            const int f = tile * S + s;
            if (f < frames) out[(long long)f * L + k] = db_of(y);
        });
}

// raw buffer resource over `bytes` bytes from p: loads past the end return 0, stores past it are dropped
__device__ __forceinline__ __amdgpu_buffer_rsrc_t brsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}

// ---- pass A: S columns x N1 rows per tile ---------------------------------------
// Column c of the frame viewed as N1 x N2: x[n1*N2 + c0 + c]. The column index is the
// fastest-varying thread coordinate in both the load and the store, so each wave reads
// and writes whole 128-B row segments (S = 16 columns x 8 B).
// Four-step twiddle W_N^(n2 k1), n2 = S*b + c: one load of the exact fp64-generated value
// from the N-entry Tfull[k1][n2] table (contiguous per 16 lanes, L2-resident). A product of
// two table values (W_N^(S b k1) x W_N^(c k1)) saved a little table space but added an
// fp32 rounding: the 64k spectrum's rms dB error on a tonal signal was 2.1x pocketfft's.
template <int L, int S, int CP = 2>   // CP: cache policy of the 256-point input loads (2 = streaming)
__device__ __forceinline__ void passA_tile(
    float2* lds, int tile, const float2* __restrict__ in, long long frameStride, int frames, const float* __restrict__ win,
    int nz, int N2, int logN, const float2* __restrict__ tw, const float2* __restrict__ tfull,
    float2* __restrict__ scratch, const float2* __restrict__ headp = nullptr, int nh = 0) {
    const int tid = threadIdx.x;
    const int c = tid % S, t = tid / S;
    constexpr int T = L / 16;
    const int nb = N2 / S;                        // column blocks per frame
    const int ntiles = nb * frames;
    if constexpr (L == 256) {
        // 256-point columns: both stages are radix 16, so the whole column is one LDS exchange.
        // Every global read is issued up front (input, window, the exact four-step twiddles of
        // this thread's 16 outputs and the WG's copy of the stage twiddles, which live in LDS),
        // so the WG waits for memory once instead of three times.
        if (tile >= ntiles) return;
        constexpr int LS = Lds<L>::LS;
        float2* twl = lds + S * LS;
        const int b = tile % nb;
        const long long f = tile / nb;
        const int col = b * S + c;
        // Buffer loads/stores: one wave-uniform resource per array and ONE per-lane byte offset
        // (o0) shared by every access of the thread; the row step r * 16 * N2 rides in the
        // scalar soffset. (Plain global accesses kept a 64-bit address pair per row live and
        // spilled at the 4-waves/SIMD register budget.)
        // split stream (fft_execute_split): frame 0 = [headp (nh) || in], frame f >= 1 at in + f stride - nh
        const float2* x = in + f * frameStride - (f > 0 ? nh : 0);
        const unsigned o0 = (unsigned)(t * N2 + col);
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)x, (short)0, 0x7fffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)win, (short)0, 0x7fffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc((void*)tfull, (short)0, 0x7fffffff, 0x00020000);
        const int rowB = T * N2 * 8;   // bytes between the rows t + 16 r and t + 16 (r + 1)
        float2 xv[16], tt[16];
        float wv[16];
        if (nh > 0 && f == 0) {   // the frame straddling two buffers (workgroup-uniform)
            // sample n comes from headp[n] (n < nh) or in[n - nh]: two range-checked loads (resources
            // of nh and nz - nh elements; the one out of range returns 0) summed, so no branch per
            // sample. The row step is in the per-lane offset: the range check ignores soffset.
            const __amdgpu_buffer_rsrc_t rh = brsrc(headp, (unsigned)nh * 8u);
            const __amdgpu_buffer_rsrc_t rb = brsrc(in, (unsigned)(nz - nh) * 8u);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const unsigned n = o0 + (unsigned)(r * T * N2);
                const bool live = (int)n < nz;
                const float2 a = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rh, n * 8, 0, 0));
                const float2 b = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rb, (n - (unsigned)nh) * 8, 0, 0));
                const float we = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rw, (live ? n : 0u) * 4, 0, 0));
                xv[r] = make_float2(a.x + b.x, a.y + b.y);
                wv[r] = live ? we : 0.0f;
            }
        } else if (nz >= L * N2) {   // no zero padding (wave-uniform)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                xv[r] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rx, o0 * 8, r * rowB, CP));
                wv[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rw, o0 * 4, r * rowB / 2, 0));
            }
        } else {              // zero-padded tail: clamped (in-bounds) loads, then select
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const unsigned n = o0 + (unsigned)(r * T * N2);
                const bool live = (int)n < nz;
                const unsigned nc = live ? n : 0u;
                const float2 xe = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rx, nc * 8, 0, 0));
                const float we = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rw, nc * 4, 0, 0));
                xv[r] = live ? xe : make_float2(0.0f, 0.0f);
                wv[r] = live ? we : 0.0f;
            }
        }
        for (int i = tid; i < L; i += S * T) twl[i] = tw[i];
        float2* tw16 = twl + L;   // twl[r t] as tw16[16 r + t]: conflict-free across t (stage_lds)
        stage16_twiddles<L>(tw16, tw, tid, S * T);
#pragma unroll
        for (int r = 0; r < 16; r++)   // exact W_N^(n2 k1), k1 = t + 16 r: same offsets as the input rows
            tt[r] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rt, o0 * 8, r * rowB, 0));
        float2 v[16];
#pragma unroll
        for (int r = 0; r < 16; r++) v[r] = make_float2(xv[r].x * wv[r], xv[r].y * wv[r]);
        float2* seq = lds + c * LS;
        stage_first<L>(seq, v, t);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; r++) v[r] = seq[pad16s<16>(t, r)];
#pragma unroll
        for (int r = 1; r < 16; r++) v[r] = cmul(v[r], tw16[16 * r + t]);
        dft16(v);
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc((void*)(scratch + (f << logN)), (short)0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float2 y = cmul(v[r], tt[r]);
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned, y), rs,
                                                  o0 * 8, r * rowB, 0);
        }
        return;
    }
    tile_loop<L, FragW>(
        lds, tw, tile, ntiles, c, t, c, t,
        [&](FragW& fr, int tile) {
            const int b = tile % nb;
            const long long f = tile / nb;
            const int col = b * S + c;
            const float2* x = in + f * frameStride;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const long long n = (long long)(t + r * T) * N2 + col;
                const bool live = n < nz;
                const long long nc = live ? n : 0;   // frame[0]: always in bounds
                fr.x[r] = x[nc];
                fr.w[r] = live ? win[nc] : 0.0f;
            }
        },
        [&](const FragW& fr, float2 (&v)[16]) {
#pragma unroll
            for (int r = 0; r < 16; r++) v[r] = make_float2(fr.x[r].x * fr.w[r], fr.x[r].y * fr.w[r]);
        },
        [&](int tile, int k1, float2 y) {
            const int b = tile % nb;
            const long long f = tile / nb;
            const float2 t0 = tfull[(long long)k1 * N2 + b * S + c];   // exact W_N^(n2 k1)
            scratch[(f << logN) + (long long)k1 * N2 + b * S + c] = cmul(y, t0);
        });
}

template <int L, int S>
__global__ __launch_bounds__(S * L / 16) __attribute__((amdgpu_waves_per_eu(4))) void fft_passA_kernel(
    const float2* __restrict__ in, long long frameStride, int frames, const float* __restrict__ win, int nz, int N2,
    int logN, const float2* __restrict__ tw, const float2* __restrict__ tfull,
    float2* __restrict__ scratch, const float2* __restrict__ headp, int nh, SideCopy side) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int ntiles = (N2 / S) * frames;
    if ((int)blockIdx.x >= ntiles) {   // spare workgroups: the caller's side copies (fft_execute_split)
        const int w = blockIdx.x - ntiles, nw = gridDim.x - ntiles;
        for (int k = 0; k < side.count; k++)
            for (int i = w * blockDim.x + threadIdx.x; i < side.n[k]; i += nw * blockDim.x) side.dst[k][i] = side.src[k][i];
        return;
    }
    passA_tile<L, S>(lds, blockIdx.x, in, frameStride, frames, win, nz, N2, logN, tw, tfull, scratch, headp, nh);
}

// ---- pass A, paired columns: S columns x N1 rows per tile, two adjacent columns per lane --
// Same transform as fft_passA_kernel with a third of its vector-memory instructions per
// element (the 64k pass A was issue-bound on them): 16-B loads of two
// adjacent columns (and an 8-B window pair), stage twiddles staged once per workgroup in
// LDS, and one 16-B load of the exact four-step twiddle pair W_N^(n2 k1) from an N-entry
// [k1][n2] table (L2-resident) instead of a product of two table values. Requires an even
// frame stride and a 16-B aligned input (checked on the host).
template <int L, int R, int NS, int V, bool T16 = false>
__device__ __forceinline__ void stage_lds_v(float2* seq0, const float2* twl, int t, const float2* tw16 = nullptr) {
    constexpr int T = L / 16, BPT = 16 / R, LS = Lds<L>::LS;
    float2 v[V][BPT][R];
#pragma unroll
    for (int q = 0; q < V; q++)
#pragma unroll
        for (int b = 0; b < BPT; b++) {
            const int j = t + b * T, jm = j % NS;
#pragma unroll
            for (int r = 0; r < R; r++) v[q][b][r] = seq0[q * LS + pad16s<L / R>(j, r)];
            if constexpr (T16 && R == 16 && NS == 16) {   // conflict-free layout (stage_lds, fft_stages.h)
#pragma unroll
                for (int r = 1; r < R; r++) v[q][b][r] = cmul(v[q][b][r], tw16[16 * r + jm]);
            } else {
#pragma unroll
                for (int r = 1; r < R; r++) v[q][b][r] = cmul(v[q][b][r], twl[r * jm * (L / (NS * R))]);
            }
            dft<R>(v[q][b]);
        }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < V; q++)
#pragma unroll
        for (int b = 0; b < BPT; b++) {
            const int j = t + b * T, idxD = (j / NS) * NS * R + (j % NS);
#pragma unroll
            for (int r = 0; r < R; r++) seq0[q * LS + pad16s<NS>(idxD, r)] = v[q][b][r];
        }
    __syncthreads();
}

template <int L, int R, int NS, int V, class Store>
__device__ __forceinline__ void stage_last_v(const float2* seq0, const float2* twl, int t, Store&& st) {
    constexpr int T = L / 16, BPT = 16 / R, LS = Lds<L>::LS;
    float2 v[V][BPT][R];
#pragma unroll
    for (int q = 0; q < V; q++)
#pragma unroll
        for (int b = 0; b < BPT; b++) {
            const int j = t + b * T, jm = j % NS;
#pragma unroll
            for (int r = 0; r < R; r++) v[q][b][r] = seq0[q * LS + pad16s<L / R>(j, r)];
#pragma unroll
            for (int r = 1; r < R; r++) v[q][b][r] = cmul(v[q][b][r], twl[r * jm * (L / (NS * R))]);
            dft<R>(v[q][b]);
        }
#pragma unroll
    for (int b = 0; b < BPT; b++) {
        const int j = t + b * T, idxD = (j / NS) * NS * R + (j % NS);
#pragma unroll
        for (int r = 0; r < R; r++) {
            float2 y[V];
#pragma unroll
            for (int q = 0; q < V; q++) y[q] = v[q][b][r];
            st(idxD + r * NS, y);
        }
    }
}

// stages 2.. of V length-L sequences (seq q at seq0 + q*LS) with LDS twiddles
template <int L, int V, class Store>
__device__ __forceinline__ void stages_rest_v(float2* seq0, const float2* twl, int t, Store&& st) {
    if constexpr (L == 64) {
        stage_last_v<L, 4, 16, V>(seq0, twl, t, st);
    } else if constexpr (L == 128) {
        stage_last_v<L, 8, 16, V>(seq0, twl, t, st);
    } else if constexpr (L == 256) {
        stage_last_v<L, 16, 16, V>(seq0, twl, t, st);
    } else {
        stage_lds_v<L, 16, 16, V>(seq0, twl, t);
        if constexpr (L == 512) stage_last_v<L, 2, 256, V>(seq0, twl, t, st);
        else if constexpr (L == 1024) stage_last_v<L, 4, 256, V>(seq0, twl, t, st);
        else if constexpr (L == 2048) stage_last_v<L, 8, 256, V>(seq0, twl, t, st);
        else stage_last_v<L, 16, 256, V>(seq0, twl, t, st);
    }
}

template <int L, int S>
__device__ __forceinline__ void passA2_tile(
    float2* lds, int tile, const float2* __restrict__ in, long long frameStride, int frames, const float* __restrict__ win,
    int nz, int N2, int logN, const float2* __restrict__ tw, const float2* __restrict__ tfull, float2* __restrict__ scratch) {
    constexpr int P = S / 2, T = L / 16, NT = P * T, LS = Lds<L>::LS;
    float2* twl = lds + S * LS;
    const int tid = threadIdx.x;
    const int cp = tid % P, t = tid / P;
    for (int i = tid; i < L; i += NT) twl[i] = tw[i];
    const int nb = N2 / S;
    const int b = tile % nb;
    const long long f = tile / nb;
    const int col = b * S + 2 * cp;
    const float2* x = in + f * frameStride;
    float4 q[16];
    float2 w[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const long long n = (long long)(t + r * T) * N2 + col;
        if (n + 1 < nz) {
            q[r] = *reinterpret_cast<const float4*>(x + n);
            w[r] = *reinterpret_cast<const float2*>(win + n);
        } else {   // zero-padded tail (n >= nz) or the one pair straddling nz
            const bool live = n < nz;
            const float2 e = x[live ? n : 0];
            const float we = live ? win[n] : 0.0f;
            q[r] = make_float4(e.x, e.y, 0.0f, 0.0f);
            w[r] = make_float2(we, 0.0f);
        }
    }
    float2 v0[16], v1[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        v0[r] = make_float2(q[r].x * w[r].x, q[r].y * w[r].x);
        v1[r] = make_float2(q[r].z * w[r].y, q[r].w * w[r].y);
    }
    dft16(v0);
    dft16(v1);
    float2* seq0 = lds + 2 * cp * LS;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        seq0[pad16lo(t, r)] = v0[r];
        seq0[LS + pad16lo(t, r)] = v1[r];
    }
    __syncthreads();
    float2* dst = scratch + (f << logN);
    stages_rest_v<L, 2>(seq0, twl, t, [&](int k1, float2 (&y)[2]) {
        const long long o = (long long)k1 * N2 + col;
        const float4 tt = *reinterpret_cast<const float4*>(tfull + o);
        const float2 a = cmul(y[0], make_float2(tt.x, tt.y)), c = cmul(y[1], make_float2(tt.z, tt.w));
        *reinterpret_cast<float4*>(dst + o) = make_float4(a.x, a.y, c.x, c.y);
    });
}

template <int L, int S>
__global__ __launch_bounds__(S / 2 * L / 16) void fft_passA2_kernel(
    const float2* __restrict__ in, long long frameStride, int frames, const float* __restrict__ win, int nz, int N2,
    int logN, const float2* __restrict__ tw, const float2* __restrict__ tfull, float2* __restrict__ scratch) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    passA2_tile<L, S>(lds, blockIdx.x, in, frameStride, frames, win, nz, N2, logN, tw, tfull, scratch);
}

// ---- 1M passes (N1 = N2 = 1024), persistent and software-pipelined ----------------------------
// The 1M column FFT needs 16 x 1024 x 8 B of LDS per tile (139 KB), so one workgroup per CU: in a
// one-shot kernel each CU alternates "load the tile" and "transform + store it", and HBM idles during
// the transform. Here each CU's workgroup walks tiles blockIdx.x, +gridDim.x, ... and issues the next
// tile's input + window loads (96 VGPRs) before it transforms the current one, so the loads fly
// during the LDS stages and the stores. The stage twiddles are staged in LDS once per workgroup, and
// the four-step twiddle W_N^(c k1) is generated in fp64 and rounded once (the same single rounding as
// a table): for column c and this thread's outputs k1 = t + 64 m, W^(c t) and W^(64 c) come from two
// 256-entry fp64 tables (W_N^(256 j), W_N^j; c t, 64 c < 2^16) and W^(c (t + 64 m)) = W^(c t)
// (W^(64 c))^m by an fp64 recurrence over m (15 products: relative error ~1e-15, far below the fp32
// rounding). That removes the 8 MB [k1][n2] table read (8 B per sample of L2 / Infinity-Cache
// traffic). Measured alternatives (rounds 2-4; kept in git history, not here): 8-column
// tiles (2.24-2.70 ms), spill-free laundered offsets (same time), the merged pass-B(c-1) + pass-A(c)
// launches (1.80 vs 1.73 ms), two workgroups per CU (2.16 ms).
__device__ __forceinline__ double2 zmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

typedef unsigned bu2 __attribute__((ext_vector_type(2)));
typedef unsigned bu4 __attribute__((ext_vector_type(4)));

// tile -> (frame, block) of the 1M pass B: G8 adjacent row blocks on one XCD at once. Workgroups x,
// x + 8, ... (same XCD, same round) take blocks b, b + 1, ..., whose 32-B dB segments share 128-B
// lines, so a line is written whole in one L2.
template <int G8>
__device__ __forceinline__ void tile_fb(int T, int nb, int& b, long long& f) {
    const int g = T / (8 * G8), w = T % (8 * G8);
    const int P = g * 8 + (w & 7), h = w >> 3;
    const int npf = nb / G8;
    f = P / npf;
    b = G8 * (P % npf) + h;
}

// ---- 1M pass B: 8 rows of 1024 per tile (two workgroups per CU), each workgroup walking tiles with
// the next tile's 16 row values per thread loaded while the current tile is transformed and stored.
// The intermediate is pass A's tile-major layout [block][k1][16 columns]: a row piece of 16 columns is
// 128 contiguous bytes. Row blocks XCD-grouped by 4 (1.93 vs 1.97 ms per C2 step; ungrouped 2.06).
// Sequence stride LSB = 1090 float2 (even; Lds<1024>::LS = 1089 elsewhere). After stage 1 a
// half-wave holds 8 sequences x 2 (read2/write2, banks by float2 index mod 16) or 4 (ds_read_b64, mod
// 32) consecutive butterflies: at stride 1089 (= 1 mod 32) sequence s and butterfly t + 1 share the
// banks of s + 1 and t -- the middle stage's accesses 2-way, the last stage's reads 4-way, 3.7
// conflict cycles per LDS instruction measured (r6e SQ counters, tools/lds_bank_model.py reproduces
// it); at 1090 (= 2 mod 32) the middle stage is conflict-free and the last stage's reads 2-way.
#ifndef SDRGPU_PB1M_LS
#define SDRGPU_PB1M_LS 1090   // (A/B builds: 1089)
#endif
constexpr int kPassB1mLS = SDRGPU_PB1M_LS;
__global__ __launch_bounds__(512) void fft_passB_1m_kernel(const float2* __restrict__ scratch, int frames, int N1, int logN,
                                                           const float2* __restrict__ tw, float* __restrict__ out) {
    constexpr int L = 1024, T = L / 16, S = 8, XG = 4, LSB = kPassB1mLS;
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    float2* twl = lds + S * LSB;   // stage twiddles, staged once per workgroup
    float2* tw16 = twl + L;                // the middle stage's, bank-conflict-free (stage_lds)
    const int tid = threadIdx.x;
    for (int i = tid; i < L; i += S * T) twl[i] = tw[i];   // (first barrier below orders both)
    for (int i = tid; i < 256; i += S * T) tw16[i] = tw[(i >> 4) * (i & 15) * (L / 256)];
    const int sF = tid / T, tF = tid % T;
    const int nb = N1 / S;
    const int ntiles = nb * frames;
    float2 fr[16];
    auto issue = [&](int tile) {
        int b;
        long long f;
        tile_fb<XG>(tile, nb, b, f);
        const __amdgpu_buffer_rsrc_t rs = brsrc(scratch + (f << logN), 0x7fffffffu);
        const unsigned o = (unsigned)((tF / 16) * L * 16 + (b * S + sF) * 16 + tF % 16) * 8u;
#pragma unroll
        for (int r = 0; r < 16; r++) fr[r] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rs, o, r * 4 * L * 16 * 8, 0));
    };
    int tile = blockIdx.x;
    if (tile < ntiles) issue(tile);
    for (; tile < ntiles; tile += gridDim.x) {
        float2 v[16];
#pragma unroll
        for (int r = 0; r < 16; r++) v[r] = fr[r];
        if (tile + (int)gridDim.x < ntiles) issue(tile + gridDim.x);
        // the LDS addresses below are loop-invariant; recomputing them per tile (laundered thread
        // index) keeps ~40 hoisted address registers from spilling the prefetched tile
        int tv = tid;
        asm volatile("" : "+v"(tv));
        const int sF2 = tv / T, tF2 = tv % T, sL2 = tv % S, tL2 = tv / S;
        __syncthreads();   // the previous tile's last LDS reads are done
        stage_first<L>(lds + sF2 * LSB, v, tF2);
        __syncthreads();
        int b;
        long long f;
        tile_fb<XG>(tile, nb, b, f);
        const __amdgpu_buffer_rsrc_t ro = brsrc(out + (f << logN) + b * S, 0x7fffffffu);
        stages_rest<L, true, LSB>(lds, twl, sL2, tL2, [&](int k2, float2 y) {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, db_of(y)), ro, (unsigned)(sL2 + N1 * k2) * 4u, 0, 0);
        }, tw16);
    }
}

// ---- 1M pass A: 16 paired columns x 1024 rows per tile, one workgroup per CU -----------------------
// The input rows are read once: streaming (slc) loads, so they do not push the 4 MB window out of L2
// (PMC fetch 18.15 -> 17.50 B/sample, C2 1.848 -> 1.798 ms). Each tile's 128 KB of output is written
// contiguously in the tile-major layout [block][k1][16] (1 KB per store instruction instead of eight
// 128-B row pieces: 1.89 vs 1.94 ms).
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(1))) void fft_passA_1m_kernel(
    const float2* __restrict__ in, long long frameStride, int frames, const float* __restrict__ win, int nz, int N2,
    int logN, const float2* __restrict__ tw, const double2* __restrict__ wt, float2* __restrict__ scratch) {
    constexpr int L = 1024, S = 16, P = S / 2, T = L / 16, NT = P * T, LS = Lds<L>::LS, CP = 2;
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    float2* twl = lds + S * LS;
    float2* tw16 = twl + L;   // the middle stage's twiddles, bank-conflict-free (stage_lds)
    const int tid = threadIdx.x;
    const int cp = tid % P, t = tid / P;
    for (int i = tid; i < L; i += NT) twl[i] = tw[i];   // (first barrier below orders both)
    for (int i = tid; i < 256; i += NT) tw16[i] = tw[(i >> 4) * (i & 15) * (L / 256)];
    const int nb = N2 / S;
    const int ntiles = nb * frames;
    // The input / window resources end at nz, so the zero-padded tail loads return 0 (nz even: a
    // column pair never straddles nz, checked on the host). The row step goes into the per-lane
    // offset, not the scalar one: the buffer range check covers voffset (+ the instruction offset)
    // only, so rows past nz addressed through soffset were NOT zeroed -- they read the next frame
    // and past the window's allocation (a first version did that: wrong and run-to-run varying
    // rows)
    const __amdgpu_buffer_rsrc_t rw = brsrc(win, (unsigned)nz * 4u);
    const int rowB = T * N2 * 8;   // bytes between rows t + 64 r and t + 64 (r + 1)
    float4 q[16];
    float2 w[16];
    auto issue = [&](int tile) {
        const int b = tile % nb;
        const long long f = tile / nb;
        const unsigned o = (unsigned)(t * N2 + b * S + 2 * cp);
        const __amdgpu_buffer_rsrc_t rx = brsrc(in + f * frameStride, (unsigned)nz * 8u);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            q[r] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, o * 8 + r * rowB, 0, CP));
            w[r] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rw, o * 4 + r * rowB / 2, 0, 0));
        }
    };
    int tile = blockIdx.x;
    if (tile < ntiles) issue(tile);
    for (; tile < ntiles; tile += gridDim.x) {
        float2 v0[16], v1[16];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            v0[r] = make_float2(q[r].x * w[r].x, q[r].y * w[r].x);
            v1[r] = make_float2(q[r].z * w[r].y, q[r].w * w[r].y);
        }
        if (tile + (int)gridDim.x < ntiles) issue(tile + gridDim.x);   // next tile's loads fly now
        dft16(v0);
        dft16(v1);
        int tv = tid;   // laundered thread index: the LDS addresses are recomputed per tile, not hoisted
        asm volatile("" : "+v"(tv));
        const int cp2 = tv % P, t2 = tv / P;
        float2* seq0 = lds + 2 * cp2 * LS;
        __syncthreads();   // the previous tile's last LDS reads are done (and twl is staged)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            seq0[pad16lo(t2, r)] = v0[r];
            seq0[LS + pad16lo(t2, r)] = v1[r];
        }
        __syncthreads();
        stage_lds_v<L, 16, 16, 2, true>(seq0, twl, t2, tw16);   // middle stage, radix 16 (two barriers inside)
        const int b = tile % nb;
        const long long f = tile / nb;
        const int col = b * S + 2 * cp;
        const __amdgpu_buffer_rsrc_t rs = brsrc(scratch + (f << logN), 0x7fffffffu);
        // Stores carry the row step in the per-lane offset and a ZERO soffset. A >64-bit buffer
        // store with an SGPR soffset gets no wait state before the next VALU write of its data
        // VGPRs (hipcc's hazard check skips that form, and two 8-B stores get merged into it): it
        // wrote already-overwritten data, rows of some lanes changing from run to run (DESIGN.md
        // §3). The offset is advanced through an opaque register so the 16 row offsets are not all
        // precomputed (register pressure).
        double2 cur[2], step[2];
#pragma unroll
        for (int qq = 0; qq < 2; qq++) {
            const int c = col + qq;
            const int e0 = c * t2, d = 64 * c;   // < 2^16
            cur[qq] = zmul(wt[e0 >> 8], wt[256 + (e0 & 255)]);
            step[qq] = zmul(wt[d >> 8], wt[256 + (d & 255)]);
        }
        // last stage (radix 4, NS = 256): outputs k1 = t + 64 m, m = b4 + 4 r, kept in registers
        float2 y[2][16];
#pragma unroll
        for (int qq = 0; qq < 2; qq++)
#pragma unroll
            for (int b4 = 0; b4 < 4; b4++) {
                const int j = t2 + b4 * T;
                float2 u[4];
#pragma unroll
                for (int r = 0; r < 4; r++) u[r] = seq0[qq * LS + pad16s<L / 4>(j, r)];
#pragma unroll
                for (int r = 1; r < 4; r++) u[r] = cmul(u[r], twl[r * j]);
                dft4v(u);
#pragma unroll
                for (int r = 0; r < 4; r++) y[qq][b4 + 4 * r] = u[r];
            }
        unsigned vo = (unsigned)(b * L * S + t * S + 2 * cp) * 8u;
#pragma unroll
        for (int m = 0; m < 16; m++) {
            const float2 a = cmul(y[0][m], make_float2((float)cur[0].x, (float)cur[0].y));
            const float2 c = cmul(y[1][m], make_float2((float)cur[1].x, (float)cur[1].y));
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bu4, make_float4(a.x, a.y, c.x, c.y)), rs, vo, 0, 0);
            vo += (unsigned)(T * S * 8);
            asm volatile("" : "+v"(vo));
            if (m < 15) {
                cur[0] = zmul(cur[0], step[0]);
                cur[1] = zmul(cur[1], step[1]);
            }
        }
    }
}

// ---- pass B: S rows of length N2 per tile, dB out, transposed store -----------------
// Stage 1 maps threads row-contiguous (coalesced row reads); the last stage maps the row
// index fastest so the transposed dB store writes S consecutive floats per k2.
// DPP move of a float: lanes outside row_mask keep `old`
template <int CTRL, int ROWMASK>
__device__ __forceinline__ float dpp_f(float old, float src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src),
                                                                 CTRL, ROWMASK, 0xF, false));
}

// lane exchange with the partner lane ^ D (D = 1, 2, 4, 8: within a 16-lane DPP row)
template <int D>
__device__ __forceinline__ float xchg(float v, int lane) {
    if constexpr (D == 1) return dpp_f<0xB1, 0xF>(v, v);             // quad_perm [1,0,3,2]
    else if constexpr (D == 2) return dpp_f<0x4E, 0xF>(v, v);        // quad_perm [2,3,0,1]
    else {                                                            // row_shr:D / row_shl:D
        const float dn = dpp_f<0x110 + D, 0xF>(v, v), up = dpp_f<0x100 + D, 0xF>(v, v);
        return (lane & D) ? dn : up;
    }
}
// one transpose-reduce step over the value pairs (v[i], v[i + H]): the lane whose bit D is 0
// keeps the lower half and takes its partner's, the other keeps the upper half
template <int D, int H>
__device__ __forceinline__ void tr_step(float (&v)[16], int lane) {
    const bool hi = (lane & D) != 0;
#pragma unroll
    for (int i = 0; i < H; i++) {
        const float send = hi ? v[i] : v[i + H];
        const float keep = hi ? v[i + H] : v[i];
        v[i] = fmaxf(keep, xchg<D>(send, lane));
    }
}

// ZM: also the waterfall's full-span zoom row (fft_scaler::doZoom with viewOffset 0 and the whole
// bandwidth in view, gui/widgets/fft_scaler.h:27-64) at factor S: out width N / S, zoom[o] = max of
// the S consecutive bins [S o, S o + S) = the bins b*S + sL of one k2, held by the S lanes sL of a
// half-wave. Each lane keeps its 16 dB values (k2 = tL + 16 r); a 16-value transpose-reduce over
// the lane bits 0..3 (DPP, VALU only) leaves in every lane the max over its 16-lane row of one r,
// one swizzle (xor 16) folds the two rows, and lanes 16..31 store the half-wave's 16 zoom values
// with one instruction.
template <int L, int S, bool ZM = false>
__device__ __forceinline__ void passB_tile(
    float2* lds, int tile, const float2* __restrict__ scratch, int frames, int N1, int logN, const float2* __restrict__ tw,
    float* __restrict__ out, float* __restrict__ zoom = nullptr) {
    constexpr int T = L / 16;
    const int tid = threadIdx.x;
    const int sF = tid / T, tF = tid % T;
    const int sL = tid % S, tL = tid / S;
    const int nb = N1 / S;
    const int ntiles = nb * frames;
    float dbv[16];   // ZM: this lane's dB values, r = k2 >> 4
    constexpr bool T16 = L >= 256;   // the radix-16 NS = 16 stage's twiddles from LDS, conflict-free
    float2* tw16 = lds + S * Lds<L>::LS;
    if constexpr (T16) stage16_twiddles<L>(tw16, tw, tid, S * T);   // (tile_loop's barrier orders it)
    tile_loop<L, FragC, T16>(
        lds, tw, tile, ntiles, sF, tF, sL, tL,
        [&](FragC& fr, int tile) {
            const int b = tile % nb;
            const long long f = tile / nb;
            const float2* src = scratch + (f << logN) + (long long)(b * S + sF) * L + tF;
#pragma unroll
            for (int r = 0; r < 16; r++) fr.x[r] = src[r * T];
        },
        [&](const FragC& fr, float2 (&v)[16]) {
#pragma unroll
            for (int r = 0; r < 16; r++) v[r] = fr.x[r];
        },
        [&](int tile, int k2, float2 y, int slot) {
            const int b = tile % nb;
            const long long f = tile / nb;
            const float d = db_of(y);
            // dB rows are written once and never read back here: streaming stores (whole 128-B
            // lines: S = 32 consecutive floats per row), so they do not evict the intermediate
            float* o = &out[(f << logN) + b * S + sL + (long long)N1 * k2];
            __builtin_nontemporal_store(d, o);
            if constexpr (ZM) dbv[slot] = d;   // stage_last<256, 16, 16>: slot r <-> k2 = tL + 16 r
        }, tw16);
    if constexpr (ZM) {
        static_assert(S == 32 && L == 256, "zoom: one half-wave per zoomed bin, k2 = tL + 16 r");
        if (tile >= ntiles) return;
        const int lane = tid & 63;
        tr_step<1, 8>(dbv, lane);
        tr_step<2, 4>(dbv, lane);
        tr_step<4, 2>(dbv, lane);
        tr_step<8, 1>(dbv, lane);
        // lane bits (b0 b1 b2 b3) now select r = 8 b0 + 4 b1 + 2 b2 + b3; fold the two rows: lane
        // i ^ 16 holds the same r (ds_swizzle xor 16 within 32 lanes: and 0x1F, xor 0x10)
        const float m = fmaxf(dbv[0], __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, dbv[0]), 0x401F)));
        if (sL >= 16) {
            const int j = sL - 16;
            const int r = ((j & 1) << 3) | ((j & 2) << 1) | ((j & 4) >> 1) | ((j & 8) >> 3);
            const int b = tile % nb;
            const long long f = tile / nb;
            zoom[(f << logN) / S + b + (long long)(N1 / S) * (tL + 16 * r)] = m;
        }
    }
}

template <int L, int S, bool ZM>
__global__ __launch_bounds__(S * L / 16) void fft_passB_kernel(
    const float2* __restrict__ scratch, int frames, int N1, int logN, const float2* __restrict__ tw,
    float* __restrict__ out, float* __restrict__ zoom) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    passB_tile<L, S, ZM>(lds, blockIdx.x, scratch, frames, N1, logN, tw, out, zoom);
}

// ---- merged launch: pass B of chunk c (first nB workgroups) + pass A of chunk c+1 --------
// The two halves share nothing (pass A writes the other scratch buffer), so one launch
// replaces two dependent kernel boundaries per chunk; the pass-B workgroups are dispatched
// first and pass A fills the CUs as they drain. The 64k split only (256 x 256, 32 columns / 32 rows, 512
// threads in both halves); the 1M split's merged form (paired pass A, pass B at 8 rows to match its 512
// threads) measured 12% SLOWER: pass B loses half its occupancy to pass A's 147 KB of LDS, so the 1M
// transform keeps separate launches.
template <bool ZM>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void fft_merged_kernel(
    int nB, const float2* __restrict__ scratchB, int framesB, float* __restrict__ outB, float* __restrict__ zoomB,
    const float2* __restrict__ in, long long frameStride, int framesA, const float* __restrict__ win, int nz,
    int logN, const float2* __restrict__ tw1, const float2* __restrict__ tw2, const float2* __restrict__ tfull,
    float2* __restrict__ scratchA) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    if ((int)blockIdx.x < nB) {
        passB_tile<256, 32, ZM>(lds, blockIdx.x, scratchB, framesB, 256, logN, tw2, outB, zoomB);
    } else {
        passA_tile<256, 32>(lds, blockIdx.x - nB, in, frameStride, framesA, win, nz, 256, logN, tw1, tfull, scratchA);
    }
}

// ---- spectrum launches that also run a VFO's first stage over the same batch ---------------
// (sdrgpu_fft_execute_vfo_dev / _zoom_vfo_dev on the 64k plan: 256 x 256, 32-column / 32-row
// tiles, 512 threads.) The IQ batch is read from HBM once: each pass-A frame's 8 column tiles are
// dispatched next to one workgroup that computes the VFO stage-1 outputs of the same 65,536
// samples (2,048 outputs of the D = 32, 143-tap decimator = 16 row-kernel segments of 128, one per
// D-lane group of its 8 waves), so the second reader of every line finds it in the Infinity Cache
// (or L2) instead of HBM (splitter.h:46-60 fans the block out with one memcpy per consumer; here no
// consumer copies it). Pass A's input loads keep the default cache policy (CP) for that reason.
// The stage's outputs are bit-identical to fir_rows_kernel's (the same fir_rows_segment; only the
// row batch is smaller, to fit the spectrum's 128-VGPR budget, which leaves the summation order
// unchanged). The launch that carries the last pass B also has the stage's history workgroup.
struct VfoWork {
    FirArgs a;       // stage 1 (vfo_stage1_prepare)
    int frame0;      // global frame index of this launch's first pass-A frame
    int hist;        // this launch's last workgroup writes the stage's next-call history
};

// The segments are those fir_rows_kernel runs (32 outputs, launch_rows): a segment's xlator phasors
// are nco(segment start) x e^{i w D r}, so the segment boundaries are part of the arithmetic, and equal
// boundaries give equal bits. Quarter q of frame g's stage-1 outputs: 16 segments of 32 outputs, one
// per D-lane group, one row batch each -- a workgroup that lives one load round, like the column
// tiles beside it.
__device__ __forceinline__ void vfo_quarter_block(const VfoWork& v, int g, int q) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long seg = (long long)(v.frame0 + g) * 64 + q * 16 + wave * 2 + (lane >> 5);
    fir_rows_segment<32, 5, true, false, 32, 32, true>(v.a, seg, lane);
}

// XCD-grouped frames. Workgroups x, x + 8, x + 16, ... run on one XCD (round-robin dispatch, speed
// only), so after the nB pass-B tiles workgroup nB + 8 k + x takes item k % 12 of frame 8 (k / 12) + x:
// a frame's 4 stage-1 quarter workgroups (items 0-3, dispatched first) and its 8 column tiles share
// one XCD's L2 and live the same load round, so the second reader of each IQ line finds it in that
// L2 instead of crossing the fabric. C5 PMC 36.7 -> 30.4 B/sample (fetch 23.5 -> 17.1), group 1.743
// -> 1.696 ms (r4g). Measured and removed: a frame's 9 workgroups consecutive over all
// XCDs (fetch 26.1 B), one whole-frame stage-1 workgroup per frame (L2 turned over), the passes
// interleaved per XCD (noise), streaming pass-A input loads (the quarters' L2 hits need the lines).
template <bool ZM>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void fft_vfo_kernel(
    int nB, const float2* __restrict__ scratchB, int framesB, float* __restrict__ outB, float* __restrict__ zoomB,
    const float2* __restrict__ in, long long frameStride, int framesA, const float* __restrict__ win, int nz,
    int logN, const float2* __restrict__ tw1, const float2* __restrict__ tw2, const float2* __restrict__ tfull,
    float2* __restrict__ scratchA, VfoWork v) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    if (v.hist && blockIdx.x == gridDim.x - 1) {   // the stage's history carry (fir.h:80)
        (void)fir_hist_block<float2, true, false>(v.a);
        return;
    }
    if ((int)blockIdx.x < nB) {
        passB_tile<256, 32, ZM>(lds, blockIdx.x, scratchB, framesB, 256, logN, tw2, outB, zoomB);
        return;
    }
    const int i = blockIdx.x - nB, k = i >> 3, kk = k % 12;
    const int g = 8 * (k / 12) + (i & 7);
    if (g >= framesA) return;   // (padding of the last group of 8 frames)
    if (kk < 4) {
        vfo_quarter_block(v, g, kk);
        return;
    }
    passA_tile<256, 32, 0>(lds, g * 8 + kk - 4, in, frameStride, framesA, win, nz, 256, logN, tw1, tfull, scratchA);
}

}  // namespace sdrgpu
