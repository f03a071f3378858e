// IF noise reduction blocks of the radio module (decoder_modules/radio/src/radio_module.h:73-79):
//   noise_reduction::FMIF     noise_reduction/fm_if.h:45-77   ("IF Noise Reduction" of WFM / NFM)
//   noise_reduction::Squelch  noise_reduction/squelch.h:33-63
// (noise_reduction::NoiseBlanker is a serial recurrence and lives in loops.hip.) This file is the host
// side: the two block structs with their launches, then the C entry points, which alone select the
// device and wait for it (blocks.h); the kernels described below are in ifnr_kernels.h.
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
#include "blocks.h"
#include "ifnr_kernels.h"

namespace sdrgpu {

struct FmifBlock : Block {
    int B = 0;
    DevBuf tab, hist[2];
    int cur = 0;
    int setup(int dev, int bins) {
        device = dev;
        in_dtype = out_dtype = SDRGPU_C64;
        SDRGPU_CHECK(tab.ensure(sizeof(float) * IF_TAB));
        for (int k = 0; k < 2; k++) SDRGPU_CHECK(hist[k].ensure(sizeof(float2) * 32));
        return set_bins(bins);
    }
    // initBuffers (fm_if.h:92-117): window and zeroed history. The caller has waited for the device: queued
    // calls still read the old table.
    int set_bins(int bins) {
        std::vector<float> t(IF_TAB);
        SDRGPU_CHECK(fmif_tables(bins, t.data(), t.data() + 32 * 32, t.data() + 2 * 32 * 32));
        SDRGPU_HIP(hipMemcpy(tab.p, t.data(), sizeof(float) * IF_TAB, hipMemcpyHostToDevice));
        B = bins;
        return reset();   // (the caller synchronises: publish_block at create, sdrgpu_fmif_set_bins)
    }
    int out_count(int count) override { return count; }
    int reset() override {   // fm_if.h:36-43
        SDRGPU_HIP(hipMemset(hist[cur].p, 0, sizeof(float2) * 32));
        return SDRGPU_OK;
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("fmif: negative count"); return SDRGPU_EARG; }
        if (count == 0) return 0;   // the history is the last B - 1 of [history || nothing]
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
        static constexpr void (*kernels[8])(FmifArgs) = {fmif_kernel<1>, fmif_kernel<2>, fmif_kernel<3>, fmif_kernel<4>,
                                                         fmif_kernel<5>, fmif_kernel<6>, fmif_kernel<7>, fmif_kernel<8>};
        hipLaunchKernelGGL(kernels[(B + 3) / 4 - 1], g, b, 0, s, a);   // k steps of 4 covering n < B (B in [3, 32])
        SDRGPU_HIP(hipGetLastError());
        cur ^= 1;
        return count;
    }
};

struct SquelchBlock : Block {
    float level = -50.0f;
    DevBuf state, part;
    int setup(int dev, double level_) {
        device = dev;
        in_dtype = out_dtype = SDRGPU_C64;
        level = (float)level_;
        SDRGPU_CHECK(state.ensure(sizeof(SquelchState)));
        return reset();
    }
    int out_count(int count) override { return count; }
    int reset() override {   // _isMute = false, cnt = 0
        SDRGPU_HIP(hipMemset(state.p, 0, sizeof(SquelchState)));
        return SDRGPU_OK;
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("squelch: negative count"); return SDRGPU_EARG; }
        if (count == 0) return 0;   // (the reference divides by zero here)
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
int fmif_bins_ok(int bins, const char* what) {
    if (bins >= SDRGPU_FMIF_MIN_BINS && bins <= SDRGPU_FMIF_MAX_BINS) return SDRGPU_OK;
    set_error("%s: bins %d outside [%d, %d]", what, bins, SDRGPU_FMIF_MIN_BINS, SDRGPU_FMIF_MAX_BINS);
    return SDRGPU_EARG;
}
}  // namespace

extern "C" int sdrgpu_fmif_create(sdrgpu_block** h, int device, int bins) {
    if (!h) { set_error("fmif_create: null handle pointer"); return SDRGPU_EARG; }
    SDRGPU_CHECK(fmif_bins_ok(bins, "fmif_create"));   // before the device is touched
    SDRGPU_SET_DEVICE(device);
    auto* f = new FmifBlock();
    return publish_block(h, f, f->setup(device, bins));
}
extern "C" int sdrgpu_fmif_set_bins(sdrgpu_block* h, int bins) {
    auto* f = h ? dynamic_cast<FmifBlock*>(h->impl) : nullptr;
    if (!f) { set_error("not an FMIF block"); return SDRGPU_EARG; }
    SDRGPU_CHECK(fmif_bins_ok(bins, "fmif_set_bins"));
    SDRGPU_CHECK(enter_block(h, true));
    SDRGPU_CHECK(f->set_bins(bins));
    SDRGPU_HIP(hipDeviceSynchronize());   // the new table and the cleared history, before the next call (blocks.h)
    return SDRGPU_OK;
}
extern "C" int sdrgpu_fmif_window(int bins, float* out) {
    const int rc = fmif_window(bins, out);
    return rc < 0 ? rc : SDRGPU_OK;
}

extern "C" int sdrgpu_squelch_create(sdrgpu_block** h, int device, double level) {
    if (!h) { set_error("squelch_create: null handle pointer"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    auto* q = new SquelchBlock();
    return publish_block(h, q, q->setup(device, level));
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
    SDRGPU_CHECK(enter_block(h, true));   // (UI-rate query: waits for the block's queued work)
    SquelchState s;
    SDRGPU_HIP(hipMemcpy(&s, q->state.p, sizeof(s), hipMemcpyDeviceToHost));
    *muted = s.muted;
    return SDRGPU_OK;
}
