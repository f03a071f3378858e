// Critically sampled M-channel polyphase channelizer (BASELINE config C4): the host side (the block
// struct, which selects no device and owns no stream, and its create function, which does: blocks.h).
// The kernels and their layout are in chan_kernels.h.
//
// Definition: channel k is FrequencyXlator(-k fs/M)
// (channel/frequency_xlator.h:43-50, exact NCO) -> DecimatingFIR<complex_t, float>(h, M)
// (filter/decimating_fir.h:45-68) with a Q*M-tap prototype h. With buf = [history || in] and
// D = M, output m of channel k is
//   y_k[m] = sum_j h[j] buf[offset + mM + j] exp(-2 pi i k n_j / M),  j = qM + r,
// and because n_j = mM + j + const, the rotation depends on r only:
//   y_k[m] = sum_c W_M^(k c) v_m[c],   v_m[(rot + r) mod M] = sum_q h[qM + r] buf[offset + (m+q)M + r].
// So one launch does, per output frame m: M branch FIRs of Q taps (the polyphase bank of
// multirate/polyphase_bank.h:32, branch r = bank phase M-1-r) and one M-point forward FFT.
// That is ~4Q + 5 log2 M flop per input sample (64 + 50 at M = 1024, Q = 16), far below the
// HBM ridge, so the kernel is HBM-bound: 8 B in + 8 B out per sample. A dense
// DFT-as-GEMM (512 flop/sample) would make it compute-bound; fp32 MFMA has no higher peak
// than packed-fp32 VALU on gfx950, so the FFT form is the faster one.
#include <algorithm>
#include <cstring>
#include <vector>
#include "sdrgpu_internal.h"
#include "blocks.h"
#include "chan_kernels.h"

namespace sdrgpu {

struct ChannelizerBlock : Block {
    int M = 0, ntaps = 0, Hp = 0, offset = 0, fpw = 256;
    int dft = 0;             // 0: LDS FFT; 1: DFT-GEMM on the matrix cores (M = 1024)
    long long phase = 0;     // absolute input index mod M of the next sample
    DevBuf taps, tw, hist[2];
    int cur = 0;

    int setup(int dev, int channels, const float* t, int n) {   // (the create function has checked the arguments)
        device = dev;
        in_dtype = out_dtype = SDRGPU_C64;
        M = channels;
        ntaps = n;
        Hp = CHAN_Q * M - 1;
        std::vector<float> pq((size_t)CHAN_Q * M, 0.0f);       // [q][r] = h[q M + r]
        for (int j = 0; j < n; j++) pq[j] = t[j];
        SDRGPU_CHECK(taps.ensure(sizeof(float) * pq.size()));
        SDRGPU_HIP(hipMemcpy(taps.p, pq.data(), sizeof(float) * pq.size(), hipMemcpyHostToDevice));
        std::vector<float2> w(M);
        for (int i = 0; i < M; i++) {
            const double a = -2.0 * M_PI * (double)i / (double)M;
            w[i] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
        SDRGPU_CHECK(tw.ensure(sizeof(float2) * M));
        SDRGPU_HIP(hipMemcpy(tw.p, w.data(), sizeof(float2) * M, hipMemcpyHostToDevice));
        for (int k = 0; k < 2; k++) SDRGPU_CHECK(hist[k].ensure(sizeof(float2) * Hp));
        return reset();
    }
    // DecimatingFIR output count (decimating_fir.h:45-68) x M channels
    int out_count(int count) override { return count > offset ? (count - offset + M - 1) / M * M : 0; }
    int reset() override {
        SDRGPU_HIP(hipMemset(hist[cur].p, 0, sizeof(float2) * Hp));
        offset = 0;
        phase = 0;
        return SDRGPU_OK;
    }
    // the kernel for (M, dft) with its dynamic LDS: sequences, twiddles, tw16
    struct Launch {
        void (*kernel)(const float2*, const float2*, int, int, const float*, long long, int, int, int, const float2*, float2*);
        size_t lds;
    };
    template <int L, bool GEMM = false>
    static Launch launch_of() { return {chan2_kernel<L, GEMM>, sizeof(float2) * (16 * Lds<L>::LS + L + 256)}; }
    Launch select_launch() const {
        if (M == 1024) return dft == 1 ? launch_of<1024, true>() : launch_of<1024>();
        return M == 512 ? launch_of<512>() : launch_of<256>();
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("channelizer: negative count"); return SDRGPU_EARG; }
        const int outN = out_count(count);
        const int frames = outN / M;
        const int H = ntaps - 1;                                   // the reference FIR's history
        if (frames > 0) {
            // buf' (history H) index b <-> padded buf index b + (Hp - H); absolute sample index
            // of buf'[b] is phase - H + b, so the NCO rotation of tap row r is (rot + r) mod M
            const long long offset0 = (long long)offset + (Hp - H);
            const int rot = (int)((((phase - H + offset) % M) + M) % M);
            const Launch l = select_launch();
            SDRGPU_HIP(hipFuncSetAttribute((const void*)l.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds));
            const int grid = (frames + fpw - 1) / fpw;
            hipLaunchKernelGGL(l.kernel, dim3(grid), dim3(M / 2), l.lds, s, hist[cur].as<float2>(), (const float2*)in, Hp, count,
                               taps.as<float>(), offset0, rot, frames, fpw, tw.as<float2>(), (float2*)out);
            SDRGPU_HIP(hipGetLastError());
        }
        if (count > 0) {
            SDRGPU_CHECK(carry_history(SDRGPU_C64, nullptr, hist[cur], in, hist[cur ^ 1], Hp, count, s));
            cur ^= 1;
        }
        offset = offset + frames * M - count;
        phase = (phase + count) % M;
        return outN;
    }
};

}  // namespace sdrgpu

using namespace sdrgpu;

extern "C" int sdrgpu_channelizer_create(sdrgpu_block** h, int device, int channels, const float* taps, int ntaps) {
    if (!h) { set_error("null out-handle"); return SDRGPU_EARG; }
    if (channels != 256 && channels != 512 && channels != 1024) {
        set_error("channelizer: %d channels unsupported (256, 512 or 1024)", channels);
        return SDRGPU_EARG;
    }
    if (!taps || ntaps < 1 || ntaps > CHAN_Q * channels) {
        set_error("channelizer: %d taps out of range [1, %d]", ntaps, CHAN_Q * channels);
        return SDRGPU_EARG;
    }
    SDRGPU_SET_DEVICE(device);
    auto* b = new ChannelizerBlock();
    return publish_block(h, b, b->setup(device, channels, taps, ntaps));
}

// C4's two forms: 0 = branch FIRs + LDS FFT (default, HBM-bound), 1 = branch FIRs + DFT as
// batched f32 MFMA GEMMs (1024 channels only)
extern "C" int sdrgpu_channelizer_set_dft(sdrgpu_block* h, int mode) {
    auto* b = h ? dynamic_cast<ChannelizerBlock*>(h->impl) : nullptr;
    if (!b) { set_error("channelizer_set_dft: not a channelizer"); return SDRGPU_EARG; }
    if (mode != 0 && mode != 1) { set_error("channelizer_set_dft: mode %d (0 FFT, 1 MFMA GEMM)", mode); return SDRGPU_EARG; }
    if (mode == 1 && b->M != 1024) { set_error("channelizer_set_dft: the MFMA GEMM form needs 1024 channels (have %d)", b->M); return SDRGPU_EARG; }
    b->dft = mode;
    return SDRGPU_OK;
}
