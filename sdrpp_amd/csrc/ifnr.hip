// IF noise reduction blocks of the radio module (decoder_modules/radio/src/radio_module.h:73-79):
//   noise_reduction::FMIF     noise_reduction/fm_if.h:45-77   ("IF Noise Reduction" of WFM / NFM)
//   noise_reduction::Squelch  noise_reduction/squelch.h:33-63
// (noise_reduction::NoiseBlanker is a serial recurrence and lives in loops.hip.)
//
// FMIF. With B = bins, w[n] = (float)nuttall(n, B - 1) and buf = [history (B - 1) || in]:
//   X_i[k] = sum_{n < B} w[n] buf[i + n] e^{-j 2 pi k n / B},   idx_i = argmax_k |X_i[k]| (lowest k on a tie),
//   out[i] = X_i[idx_i] e^{+j 2 pi idx_i floor(B/2) / B}
// (the reference runs a forward FFTW plan, keeps the peak bin and reads sample B/2 of an
// unnormalised backward plan, per sample). Every output is independent: count x B x B complex
// MACs = a GEMM with the samples as rows and the bins as columns, on the f32 matrix cores
// (v_mfma_f32_16x16x4_f32, layout as fir_mfma_kernel in fir_mfma.h):
//   A[i][n] = buf[o + i + n]   Toeplitz rows of the span staged in LDS: lane (i = lane & 15,
//                              kk = lane >> 4) reads X[o + i + 4 s + kk] at k step s, consecutive
//                              addresses across lanes (conflict-free);
//   B[n][k] = c[n][k] = w[n] e^{-j 2 pi k n / B}   host-built (host_design.cpp fmif_tables: fp64,
//                              rounded once), zero-padded to 4 | n and to 16 or 32 bins, held in
//                              registers for the whole workgroup;
//   four real products per complex product (re += xr cr - xi ci, im += xr ci + xi cr).
// Accumulator element e of a lane is sample 4 (lane >> 4) + e, bin lane & 15 of the tile: the 16
// bins of one sample sit across one 16-lane DPP row. The argmax is a row reduction over
// (|X|^2, k): the two bin tiles are merged in registers, a DPP row_ror max gives every lane the
// row's largest |X|^2, a DPP min over the k of the lanes that hold it gives the lowest such k.
// Squared magnitudes are compared (the reference compares sqrtf of them: same order up to
// rounding; the tests gate on decidable samples). Padding bins carry -1 and never win; an
// all-zero window picks k = 0. The winning lane multiplies by ph[k] and the outputs leave
// through LDS with one coalesced vector store per output. 8 B^2 real flop per sample on padded
// B (8192 at B = 32) against 16 B of traffic: bound by the matrix cores, not by memory.
//
// No atomics; the MFMA chain of an output runs over n in the same order wherever the output
// falls in a tile or a call, so results are bit-identical from run to run and independent of how
// a stream is cut into calls (for finite input: the zero-padded n read real samples times 0).
// History as in the FIR block: two device buffers, the launch's last workgroup writes the next
// call's history = the last B - 1 of [history || in]; tiles fetch [history || in] element-wise
// (the span of a tile is 1056 elements against ~33k MFMA cycles: not worth an interior path).
//
// Squelch: per call, level = 20 log10f(sum |x| / count), then the reference's state machine
// (muted, cnt) in device memory and the gated copy, all enqueued on the caller's stream (no
// host synchronise): per-workgroup partial sums in a fixed order, one workgroup that sums the
// partials (fixed-order tree) and takes the decision, one copy-or-zero pass that reads it.
#include <algorithm>
#include <cmath>
#include <vector>
#include "sdrgpu_internal.h"

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
// one wave's LDS stores visible to its other lanes (as chan_dft_gemm in channelizer.hip)
__device__ __forceinline__ void wave_lds_handoff() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
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

struct FmifBlock : Block {
    int B = 0;
    DevBuf tab, hist[2];
    int cur = 0;
    int setup(int dev, int bins) {
        device = dev;
        in_dtype = out_dtype = SDRGPU_C64;
        SDRGPU_CHECK(init_stream());
        SDRGPU_CHECK(tab.ensure(sizeof(float) * IF_TAB));
        for (int k = 0; k < 2; k++) SDRGPU_CHECK(hist[k].ensure(sizeof(float2) * 32));
        return set_bins(bins);
    }
    int set_bins(int bins) {   // initBuffers (fm_if.h:92-117): window and zeroed history
        std::vector<float> t(IF_TAB);
        SDRGPU_CHECK(fmif_tables(bins, t.data(), t.data() + 32 * 32, t.data() + 2 * 32 * 32));
        SDRGPU_SET_DEVICE(device);
        SDRGPU_HIP(hipDeviceSynchronize());   // queued calls still read the old table
        SDRGPU_HIP(hipMemcpy(tab.p, t.data(), sizeof(float) * IF_TAB, hipMemcpyHostToDevice));
        B = bins;
        return reset();
    }
    int out_count(int count) override { return count; }
    int reset() override {   // fm_if.h:36-43
        SDRGPU_SET_DEVICE(device);
        SDRGPU_HIP(hipMemset(hist[cur].p, 0, sizeof(float2) * 32));
        SDRGPU_HIP(hipDeviceSynchronize());   // done before a call on any (non-blocking) stream reads it
        return SDRGPU_OK;
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("fmif: negative count"); return SDRGPU_EARG; }
        if (count == 0) return 0;   // the history is the last B - 1 of [history || nothing]
        SDRGPU_SET_DEVICE(device);
        FmifArgs a;
        a.in = (const float2*)in;
        a.out = (float2*)out;
        a.hist = hist[cur].as<float2>();
        a.histNext = hist[cur ^ 1].as<float2>();
        a.tab = tab.as<float>();
        a.count = count;
        a.B = B;
        a.ntiles = (int)(((long long)count + IF_TM - 1) / IF_TM);
        const dim3 g(a.ntiles + 1), b(IF_NT);
        switch ((B + 3) / 4) {
        case 1: hipLaunchKernelGGL(fmif_kernel<1>, g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL(fmif_kernel<2>, g, b, 0, s, a); break;
        case 3: hipLaunchKernelGGL(fmif_kernel<3>, g, b, 0, s, a); break;
        case 4: hipLaunchKernelGGL(fmif_kernel<4>, g, b, 0, s, a); break;
        case 5: hipLaunchKernelGGL(fmif_kernel<5>, g, b, 0, s, a); break;
        case 6: hipLaunchKernelGGL(fmif_kernel<6>, g, b, 0, s, a); break;
        case 7: hipLaunchKernelGGL(fmif_kernel<7>, g, b, 0, s, a); break;
        default: hipLaunchKernelGGL(fmif_kernel<8>, g, b, 0, s, a); break;
        }
        SDRGPU_HIP(hipGetLastError());
        cur ^= 1;
        return count;
    }
};

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

struct SquelchBlock : Block {
    float level = -50.0f;
    DevBuf state, part;
    int setup(int dev, double level_) {
        device = dev;
        in_dtype = out_dtype = SDRGPU_C64;
        level = (float)level_;
        SDRGPU_CHECK(init_stream());
        SDRGPU_CHECK(state.ensure(sizeof(SquelchState)));
        return reset();
    }
    int out_count(int count) override { return count; }
    int reset() override {   // _isMute = false, cnt = 0
        SDRGPU_SET_DEVICE(device);
        SDRGPU_HIP(hipMemset(state.p, 0, sizeof(SquelchState)));
        SDRGPU_HIP(hipDeviceSynchronize());   // done before a call on any (non-blocking) stream reads it
        return SDRGPU_OK;
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("squelch: negative count"); return SDRGPU_EARG; }
        if (count == 0) return 0;   // (the reference divides by zero here)
        SDRGPU_SET_DEVICE(device);
        const int nparts = (int)(((long long)count + SQ_CHUNK - 1) / SQ_CHUNK);
        SDRGPU_CHECK(part.ensure(sizeof(float) * nparts));
        hipLaunchKernelGGL(squelch_partial_kernel, dim3(nparts), dim3(SQ_NT), 0, s, (const float2*)in, count, part.as<float>());
        hipLaunchKernelGGL(squelch_decide_kernel, dim3(1), dim3(SQ_NT), 0, s, part.as<float>(), nparts, count, level,
                           state.as<SquelchState>());
        hipLaunchKernelGGL(squelch_gate_kernel, dim3((unsigned)(((long long)count + SQ_NT - 1) / SQ_NT)), dim3(SQ_NT), 0, s,
                           (const float2*)in, (float2*)out, count, state.as<SquelchState>());
        SDRGPU_HIP(hipGetLastError());
        return count;
    }
};
}  // namespace sdrgpu

using namespace sdrgpu;

namespace {
int wrap_block(sdrgpu_block** h, Block* b, int rc) {
    if (rc < 0) { delete b; return rc; }
    *h = new sdrgpu_block{b};
    return SDRGPU_OK;
}
int fmif_bins_ok(int bins, const char* what) {
    if (bins >= SDRGPU_FMIF_MIN_BINS && bins <= SDRGPU_FMIF_MAX_BINS) return SDRGPU_OK;
    set_error("%s: bins %d outside [%d, %d]", what, bins, SDRGPU_FMIF_MIN_BINS, SDRGPU_FMIF_MAX_BINS);
    return SDRGPU_EARG;
}
}  // namespace

extern "C" int sdrgpu_fmif_create(sdrgpu_block** h, int device, int bins) {
    if (!h) { set_error("fmif_create: null handle pointer"); return SDRGPU_EARG; }
    SDRGPU_CHECK(fmif_bins_ok(bins, "fmif_create"));   // before the device is touched
    auto* f = new FmifBlock();
    return wrap_block(h, f, f->setup(device, bins));
}
extern "C" int sdrgpu_fmif_set_bins(sdrgpu_block* h, int bins) {
    auto* f = h ? dynamic_cast<FmifBlock*>(h->impl) : nullptr;
    if (!f) { set_error("not an FMIF block"); return SDRGPU_EARG; }
    SDRGPU_CHECK(fmif_bins_ok(bins, "fmif_set_bins"));
    return f->set_bins(bins);
}
extern "C" int sdrgpu_fmif_window(int bins, float* out) {
    const int rc = fmif_window(bins, out);
    return rc < 0 ? rc : SDRGPU_OK;
}

extern "C" int sdrgpu_squelch_create(sdrgpu_block** h, int device, double level) {
    if (!h) { set_error("squelch_create: null handle pointer"); return SDRGPU_EARG; }
    auto* q = new SquelchBlock();
    return wrap_block(h, q, q->setup(device, level));
}
extern "C" int sdrgpu_squelch_set_level(sdrgpu_block* h, double level) {
    auto* q = h ? dynamic_cast<SquelchBlock*>(h->impl) : nullptr;
    if (!q) { set_error("not a squelch block"); return SDRGPU_EARG; }
    q->level = (float)level;
    return SDRGPU_OK;
}
extern "C" int sdrgpu_squelch_get_muted(sdrgpu_block* h, int* muted) {
    auto* q = h ? dynamic_cast<SquelchBlock*>(h->impl) : nullptr;
    if (!q || !muted) { set_error("squelch_get_muted: bad argument"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(q->device);
    SquelchState s;
    SDRGPU_HIP(hipDeviceSynchronize());   // (UI-rate query: waits for the block's queued work)
    SDRGPU_HIP(hipMemcpy(&s, q->state.p, sizeof(s), hipMemcpyDeviceToHost));
    *muted = s.muted;
    return SDRGPU_OK;
}
