// Host side of the stream banks (the kernels, the layout and the kernel form are in bank_kernels.h, which
// also says why this file is built with -ffp-contract=off): S independent streams with shared
// parameters, element m of stream k at x[m * S + k], one launch per block and call.
//   BankQuad, BankFir        demod::Quadrature, filter::FIR<D, float> per stream
//   BankFastAgc, BankCostas, BankMm   loop::FastAGC<T>, loop::Costas<ORDER>, clock_recovery::MM<T> per stream
//   BankPll                  loop::PLL, loop::CarrierTrackingPLL, loop::MeteorCostas (with demod::Meteor's stagger) per stream
//   BankAgc, BankDcb, BankDeemp      loop::AGC<T>, correction::DCBlocker<T>, filter::Deemphasis<float> per stream
//   BankSquelch, BankMag     noise_reduction::Squelch per stream; volk_32fc_magnitude_32f over the flat stream
//   BankXlator               channel::FrequencyXlator per stream on the single-stream NCO; also as translate -> real part
//   BankRate, BankCopy       multirate::PolyphaseResampler<T> / filter::DecimatingFIR<D, float> per stream
//                            (bank_rate_kernels.h); the copy of a ratio of 1
//   BankCfir, BankStereoDec, BankMonoPairs   filter::FIR<complex_t, complex_t> per stream; the stereo decoder of
//                            demod::BroadcastFM (pilot filter -> PLL -> matrix) and its mono -> pairs (bank_wfm_kernels.h)
//   BankChain                demod::PSK<ORDER> / demod::GFSK / demod::Meteor per stream (the constants of symsync.hip),
//                            demod::FM<float> / demod::AM<float> / demod::SSB<float> / demod::CW<float> per stream
//                            (those of blocks.hip / loops.hip), demod::BroadcastFM per stream (those of loops.hip),
//                            multirate::PowerDecimator<T> / multirate::RationalResampler<T> per stream
// Top to bottom: the Bank base and its handle, the blocks (each: configure = the argument checks and the
// parameters, host only; init = device state; reset; run = its launch), the C entry points.
// A create function checks every argument (configure, of a chain: of all its stages) before it selects
// the device. Banks are not Blocks: sdrgpu_block_process sizes its buffers as count * esize and knows
// nothing of rows.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>
#include "sdrgpu_internal.h"
#include "bank_kernels.h"
#include "bank_audio_kernels.h"
#include "bank_rate_kernels.h"
#include "bank_wfm_kernels.h"
#include "blocks.h"
#include "symsync_args.h"

namespace sdrgpu {

struct Bank {
    int device = 0, S = 1;
    int in_dtype = SDRGPU_C64, out_dtype = SDRGPU_C64;
    hipStream_t own = nullptr;   // the handle's own stream (a chain's stages have none)
    StreamOrder order;           // entry points only, as Block::order
    PinnedBuf pin_in, pin_out;
    DevBuf dev_in, dev_out;
    int lastRows = 0;
    virtual ~Bank() {
        if (own) (void)hipStreamDestroy(own);
    }
    // device state (allocations, uploads, reset); the device is selected
    virtual int init() = 0;
    virtual int reset() = 0;
    // frames rows at `in` -> rows at `out`, asynchronous on s unless the block says otherwise; returns the rows
    virtual int run(const void* in, int frames, void* out, hipStream_t s) = 0;
    // the rows the next run() of `frames` rows writes, from the state as it is (which stays): exact, except for
    // data-dependent counts (MM), where it is the capacity. Past rows_limit(): some stage's rows do not fit the index.
    virtual long long out_rows(int frames) const { return frames; }
    // data-dependent per-stream counts (MM): rows past a stream's count keep what `out` held
    virtual bool ragged() const { return false; }
    virtual void counts(int* c) const { std::fill(c, c + S, lastRows); }
    // streams and the index bounds of the kernels: state words f * S + k (MMW_WORDS) and history rows
    // (up to SDRGPU_MM_MAX_TAPS - 1) are int
    static bool streams_ok(int streams) {
        if (streams < 1 || streams > INT_MAX / 64) { set_error("bank: %d streams outside [1, %d]", streams, INT_MAX / 64); return false; }
        return true;
    }
    long long rows_limit() const { return INT_MAX / S; }
    // rows in and rows out of a call
    bool frames_ok(int frames) const {
        if (frames < 0 || frames > rows_limit() || out_rows(frames) > rows_limit()) {
            set_error("bank: %d frames of %d streams, or the rows they yield, do not fit the kernels' int index", frames, S);
            return false;
        }
        return true;
    }
};

// a state buffer's initial words, uploaded on the null stream (the entry point synchronises: blocks.h)
template <typename T>
static int upload(DevBuf& b, const std::vector<T>& v) {
    SDRGPU_CHECK(b.ensure(sizeof(T) * v.size()));
    SDRGPU_HIP(hipMemcpy(b.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return SDRGPU_OK;
}
static dim3 waves_of(int S) { return dim3((S + BANK_W - 1) / BANK_W); }   // one wave per 64 streams, none idle

// ------------------------------------------------------------------ Quadrature
struct BankQuad : Bank {
    float invDev = 1.0f;
    DevBuf prev[2];   // the streams' last samples: [cur] read by the next call, [cur ^ 1] written by it
    int cur = 0;
    int configure(int streams, double deviationRad) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        S = streams;
        in_dtype = SDRGPU_C64;
        out_dtype = SDRGPU_F32;
        invDev = (float)(1.0 / deviationRad);
        return SDRGPU_OK;
    }
    int init() override {
        for (auto& b : prev) SDRGPU_CHECK(b.ensure(sizeof(float2) * S));
        return reset();
    }
    int reset() override {
        SDRGPU_HIP(hipMemset(prev[cur].p, 0, sizeof(float2) * S));
        return SDRGPU_OK;
    }
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        const int n = frames * S;
        hipLaunchKernelGGL(bank_quad_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const float2*)in, (float*)out, n, S,
                           prev[cur].as<float2>(), prev[cur ^ 1].as<float2>(), invDev);
        SDRGPU_HIP(hipGetLastError());
        cur ^= 1;
        return frames;
    }
};

// ------------------------------------------------------------------------- FIR
struct BankFir : Bank {
    std::vector<float> taps;
    DevBuf tapsDev, hist[2];
    int cur = 0;
    int configure(int streams, int dtype, const float* t, int ntaps) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        if (!real_or_complex(dtype) || !t || ntaps < 1 || (long long)(ntaps - 1) * streams > INT_MAX) {
            set_error("bank_fir: dtype %d not F32 / C64, no taps, or %d taps of %d streams beyond the int index", dtype, ntaps, streams);
            return SDRGPU_EARG;
        }
        S = streams;
        in_dtype = out_dtype = dtype;
        taps.assign(t, t + ntaps);
        return SDRGPU_OK;
    }
    int HS() const { return ((int)taps.size() - 1) * S; }
    int init() override {
        SDRGPU_CHECK(upload(tapsDev, taps));
        for (auto& b : hist) SDRGPU_CHECK(b.ensure(esize(in_dtype) * (size_t)std::max(HS(), 1)));
        return reset();
    }
    int reset() override {
        SDRGPU_HIP(hipMemset(hist[cur].p, 0, hist[cur].bytes));
        return SDRGPU_OK;
    }
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        const int n = frames * S, T = (int)taps.size();
        if (in_dtype == SDRGPU_C64)
            hipLaunchKernelGGL(bank_fir_kernel<float2>, dim3((n + 255) / 256), dim3(256), 0, s, (const float2*)in, (float2*)out, n, S,
                               HS(), tapsDev.as<float>(), T, hist[cur].as<float2>());
        else
            hipLaunchKernelGGL(bank_fir_kernel<float>, dim3((n + 255) / 256), dim3(256), 0, s, (const float*)in, (float*)out, n, S,
                               HS(), tapsDev.as<float>(), T, hist[cur].as<float>());
        SDRGPU_HIP(hipGetLastError());
        if (HS() > 0) {
            SDRGPU_CHECK(carry_history(in_dtype, nullptr, hist[cur], in, hist[cur ^ 1], HS(), n, s));
            cur ^= 1;
        }
        return frames;
    }
};

// --------------------------------------------------------------------- FastAGC
struct BankFastAgc : Bank {
    FastAgcParams p{};
    float initGain = 1.0f;
    DevBuf state;   // gain[S]
    int configure(int streams, int dtype, double setPoint, double maxGain, double rate, double initGain_) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        if (!real_or_complex(dtype)) { set_error("bank_fast_agc: dtype %d not F32 / C64", dtype); return SDRGPU_EARG; }
        S = streams;
        in_dtype = out_dtype = dtype;
        fast_agc_params(p, setPoint, maxGain, rate);
        initGain = (float)initGain_;
        return SDRGPU_OK;
    }
    int init() override { return reset(); }
    int reset() override { return upload(state, std::vector<float>(S, initGain)); }   // fast_agc.h:54-58
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        if (in_dtype == SDRGPU_C64)
            hipLaunchKernelGGL(bank_fast_agc_kernel<float2>, waves_of(S), dim3(BANK_W), 0, s, (const float2*)in, (float2*)out, frames, S, p,
                               state.as<float>());
        else
            hipLaunchKernelGGL(bank_fast_agc_kernel<float>, waves_of(S), dim3(BANK_W), 0, s, (const float*)in, (float*)out, frames, S, p,
                               state.as<float>());
        SDRGPU_HIP(hipGetLastError());
        return frames;
    }
};

// ---------------------------------------------------------------------- Costas
struct BankCostas : Bank {
    int order = 2;
    PclParams p{};
    float initPhase = 0.0f, initFreq = 0.0f;
    DevBuf state;   // phase[S], freq[S]
    int configure(int streams, int order_, double bandwidth, double initPhase_, double initFreq_, double minFreq, double maxFreq) {
        if (!streams_ok(streams) || !costas_args_ok(order_, bandwidth, initPhase_, initFreq_, minFreq, maxFreq)) return SDRGPU_EARG;
        S = streams;
        in_dtype = out_dtype = SDRGPU_C64;
        order = order_;
        critically_damped(bandwidth, &p.alpha, &p.beta);
        p.minFreq = (float)minFreq;
        p.maxFreq = (float)maxFreq;
        initPhase = (float)initPhase_;
        initFreq = (float)initFreq_;
        return SDRGPU_OK;
    }
    int init() override { return reset(); }
    int reset() override {   // pll.h:55-62
        std::vector<float> st(2 * (size_t)S, initPhase);
        std::fill(st.begin() + S, st.end(), initFreq);
        return upload(state, st);
    }
    template <int ORDER>
    void run_t(const void* in, int frames, void* out, hipStream_t s) {
        hipLaunchKernelGGL(bank_costas_kernel<ORDER>, waves_of(S), dim3(BANK_W), 0, s, (const float2*)in, (float2*)out, frames, S, p,
                           state.as<float>());
    }
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        if (order == 2) run_t<2>(in, frames, out, s);
        else if (order == 4) run_t<4>(in, frames, out, s);
        else run_t<8>(in, frames, out, s);
        SDRGPU_HIP(hipGetLastError());
        return frames;
    }
};

// ---------------------------------------- MeteorCostas, PLL, CarrierTrackingPLL
// the three other PLLs of the reference on BankCostas's configuration and state
enum class PllKind { Meteor, Pll, Carrier };
struct BankPll : BankCostas {
    PllKind kind = PllKind::Pll;
    int broken = 0, oqpsk = 0;
    DevBuf lastI;   // lastI[S], demod::Meteor's stagger carry per stream: 0 at create, a reset keeps it
    int configure(int streams, PllKind kind_, double bandwidth, int broken_, int oqpsk_, double initPhase_, double initFreq_,
                  double minFreq, double maxFreq) {
        kind = kind_;
        broken = broken_ ? 1 : 0;
        oqpsk = oqpsk_ ? 1 : 0;
        return BankCostas::configure(streams, 4, bandwidth, initPhase_, initFreq_, minFreq, maxFreq);
    }
    int init() override {
        if (kind == PllKind::Meteor) SDRGPU_CHECK(upload(lastI, std::vector<float>(S, 0.0f)));
        return reset();
    }
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        if (kind == PllKind::Meteor)
            hipLaunchKernelGGL(bank_meteor_costas_kernel, waves_of(S), dim3(BANK_W), 0, s, (const float2*)in, (float2*)out, frames, S, p,
                               broken, oqpsk, state.as<float>(), lastI.as<float>());
        else if (kind == PllKind::Carrier)
            hipLaunchKernelGGL(bank_carrier_pll_kernel<true>, waves_of(S), dim3(BANK_W), 0, s, (const float2*)in, (float2*)out, frames, S,
                               pll_params(p), state.as<float>());
        else
            hipLaunchKernelGGL(bank_carrier_pll_kernel<false>, waves_of(S), dim3(BANK_W), 0, s, (const float2*)in, (float2*)out, frames, S,
                               pll_params(p), state.as<float>());
        SDRGPU_HIP(hipGetLastError());
        return frames;
    }
};

// -------------------------------------------------------------------------- MM
struct BankMm : Bank {
    MmParams p{};
    double omega = 0.0;
    std::vector<float> interp;
    DevBuf state, hist, interpDev;   // MMW_WORDS x S words; (T - 1) x S elements; P x T floats
    PinnedBuf countBuf;              // the call's per-stream counts, read back at the end of run()
    std::vector<int> last;           // ... and kept for sdrgpu_bank_out_counts
    int configure(int streams, int dtype, double omega_, double omegaGain, double muGain, double rel, int P, int T) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        if (!real_or_complex(dtype)) { set_error("bank_mm: dtype %d not F32 / C64", dtype); return SDRGPU_EARG; }
        if (!mm_args_ok(omega_, omegaGain, muGain, rel, P, T)) return SDRGPU_EARG;
        S = streams;
        in_dtype = out_dtype = dtype;
        omega = omega_;
        mm_pcl_params(p, omega, omegaGain, muGain, rel);
        p.P = P;
        p.T = T;
        p.inStride = 1;
        p.modulus = 2;
        interp.resize((size_t)P * T);
        SDRGPU_CHECK(mm_interp_bank(P, T, interp.data()));
        last.assign(S, 0);
        return SDRGPU_OK;
    }
    bool ragged() const override { return true; }
    void counts(int* c) const override { std::copy(last.begin(), last.end(), c); }
    size_t lds_bytes() const {
        const size_t tile = (size_t)(BANK_F + p.T - 1) * BANK_W * esize(in_dtype);
        return tile + (p.P * p.T <= MM_LDS_BANK ? sizeof(float) * interp.size() : 0);
    }
    int init() override {
        SDRGPU_CHECK(upload(interpDev, interp));
        SDRGPU_CHECK(hist.ensure(esize(in_dtype) * (size_t)std::max((p.T - 1) * S, 1)));
        SDRGPU_CHECK(countBuf.ensure(sizeof(int) * S));
        SDRGPU_HIP(hipMemset(hist.p, 0, hist.bytes));   // (the reference's work buffer starts uninitialised)
        return reset();
    }
    int reset() override {   // mm.h:87-98: the state, not the history
        std::vector<int> st((size_t)MMW_WORDS * S, 0);
        const float f = (float)omega;
        int fbits;
        std::memcpy(&fbits, &f, sizeof(f));
        std::fill(st.begin() + (size_t)MMW_FREQ * S, st.begin() + (size_t)(MMW_FREQ + 1) * S, fbits);
        std::fill(last.begin(), last.end(), 0);
        return upload(state, st);
    }
    // as MmBlock::run: the data-dependent counts are the one wait of the call; returns the largest
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        std::fill(last.begin(), last.end(), 0);
        if (frames == 0) return 0;
        if (in_dtype == SDRGPU_C64)
            hipLaunchKernelGGL(bank_mm_kernel<float2>, waves_of(S), dim3(BANK_W), lds_bytes(), s, (const float2*)in, frames, S, (float2*)out,
                               p, interpDev.as<float>(), hist.as<float2>(), state.as<int>());
        else
            hipLaunchKernelGGL(bank_mm_kernel<float>, waves_of(S), dim3(BANK_W), lds_bytes(), s, (const float*)in, frames, S, (float*)out, p,
                               interpDev.as<float>(), hist.as<float>(), state.as<int>());
        SDRGPU_HIP(hipGetLastError());
        SDRGPU_HIP(hipMemcpyAsync(countBuf.p, state.as<int>() + (size_t)MMW_COUNT * S, sizeof(int) * S, hipMemcpyDeviceToHost, s));
        SDRGPU_HIP(hipStreamSynchronize(s));
        const int* c = reinterpret_cast<const int*>(countBuf.p);
        last.assign(c, c + S);
        return *std::max_element(last.begin(), last.end());
    }
};

// ------------------------------------------------------------------------- AGC
// tiles x waves, folded into grid.x (bank_tile_of_block)
static dim3 tiles_by_waves(int frames, int S) { return dim3((unsigned)((frames + BANK_F - 1) / BANK_F) * waves_of(S).x); }

struct BankAgc : Bank {
    AgcParams p{};
    float initGain = 1.0f;
    DevBuf state, tm;   // amp[S], gain[S]; the tile maxima of a call (grows on demand)
    bool pending = false;
    float pendingGain = 0.0f;
    int configure(int streams, int dtype, double setPoint, double attack, double decay, double maxGain, double maxOutputAmp,
                  double initGain_, int enabled) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        if (!real_or_complex(dtype)) { set_error("bank_agc: dtype %d not F32 / C64", dtype); return SDRGPU_EARG; }
        S = streams;
        in_dtype = out_dtype = dtype;
        p.setPoint = (float)setPoint;   // AGC::init (agc.h:13-26): members are float
        p.attack = (float)attack;
        p.invAttack = 1.0f - p.attack;
        p.decay = (float)decay;
        p.invDecay = 1.0f - p.decay;
        p.maxGain = (float)maxGain;
        p.maxOutputAmp = (float)maxOutputAmp;
        p.enabled = enabled ? 1 : 0;
        initGain = (float)initGain_;
        return SDRGPU_OK;
    }
    int init() override { return reset(); }
    int reset() override {   // agc.h:81-86
        std::vector<float> st(2 * (size_t)S, p.setPoint / initGain);
        std::fill(st.begin() + S, st.end(), (p.maxGain < initGain) ? p.maxGain : initGain);
        pending = false;
        return upload(state, st);
    }
    void set_gain(float g) {   // agc.h:31-35, latched by the next call that has rows
        pending = true;
        pendingGain = g;
    }
    template <typename DT>
    void run_t(const void* in, int frames, void* out, hipStream_t s) {
        if (p.enabled)
            hipLaunchKernelGGL(bank_tile_max_kernel<DT>, tiles_by_waves(frames, S), dim3(BANK_W), 0, s, (const DT*)in, frames, S,
                               tm.as<float>());
        hipLaunchKernelGGL(bank_agc_kernel<DT>, waves_of(S), dim3(BANK_W), 0, s, (const DT*)in, (DT*)out, frames, S, p,
                           state.as<float>(), tm.as<float>(), pending ? 1 : 0, pendingGain);
    }
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        if (p.enabled) SDRGPU_CHECK(tm.ensure(sizeof(float) * (size_t)((frames + BANK_F - 1) / BANK_F) * S));
        if (in_dtype == SDRGPU_C64) run_t<float2>(in, frames, out, s);
        else run_t<float>(in, frames, out, s);
        SDRGPU_HIP(hipGetLastError());
        pending = false;
        return frames;
    }
};

// ------------------------------------------------------------------- DCBlocker
struct BankDcb : Bank {
    float rate = 0.0f;
    DevBuf state;   // offset[S] (C64: re[S], im[S])
    int configure(int streams, int dtype, double rate_) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        if (!real_or_complex(dtype)) { set_error("bank_dc_blocker: dtype %d not F32 / C64", dtype); return SDRGPU_EARG; }
        S = streams;
        in_dtype = out_dtype = dtype;
        rate = (float)rate_;
        return SDRGPU_OK;
    }
    int init() override { return reset(); }
    int reset() override { return upload(state, std::vector<float>(2 * (size_t)S, 0.0f)); }   // dc_blocker.h:45-48
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        if (in_dtype == SDRGPU_C64)
            hipLaunchKernelGGL(bank_dcb_kernel<float2>, waves_of(S), dim3(BANK_W), 0, s, (const float2*)in, (float2*)out, frames, S, rate,
                               state.as<float>());
        else
            hipLaunchKernelGGL(bank_dcb_kernel<float>, waves_of(S), dim3(BANK_W), 0, s, (const float*)in, (float*)out, frames, S, rate,
                               state.as<float>());
        SDRGPU_HIP(hipGetLastError());
        return frames;
    }
};

// ------------------------------------------------------------------ Deemphasis
// filter::Deemphasis<float> (channels = 1) or <stereo_t> (2: C64 rows of (l, r)) per stream
struct BankDeemp : Bank {
    float alpha = 1.0f;
    int channels = 1;
    DevBuf state;   // lastOut[S]; stereo: l[S], r[S]
    int configure(int streams, double tau, double samplerate, bool stereo) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        if (!(samplerate > 0)) { set_error("bank_deemphasis: samplerate %g not positive", samplerate); return SDRGPU_EARG; }
        S = streams;
        channels = stereo ? 2 : 1;
        in_dtype = out_dtype = stereo ? SDRGPU_C64 : SDRGPU_F32;
        const float dt = (float)(1.0f / samplerate);   // updateAlpha (deephasis.h:91-94), as sdrgpu_deemphasis_create
        alpha = (float)((double)dt / (tau + (double)dt));
        return SDRGPU_OK;
    }
    int init() override { return reset(); }
    int reset() override { return upload(state, std::vector<float>((size_t)channels * S, 0.0f)); }
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        if (channels == 2)
            hipLaunchKernelGGL((bank_deemp_kernel<2, float2>), waves_of(S), dim3(BANK_W), 0, s, (const float2*)in, (float2*)out, frames, S,
                               alpha, state.as<float>());
        else
            hipLaunchKernelGGL((bank_deemp_kernel<1, float>), waves_of(S), dim3(BANK_W), 0, s, (const float*)in, (float*)out, frames, S,
                               alpha, state.as<float>());
        SDRGPU_HIP(hipGetLastError());
        return frames;
    }
};

// --------------------------------------------------------------------- Squelch
struct BankSquelch : Bank {
    float level = -50.0f;
    DevBuf state, part;   // muted[S], cnt[S]; the tile sums of a call (grows on demand)
    int configure(int streams, double level_) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        S = streams;
        in_dtype = out_dtype = SDRGPU_C64;
        level = (float)level_;
        return SDRGPU_OK;
    }
    int init() override { return reset(); }
    int reset() override { return upload(state, std::vector<int>(2 * (size_t)S, 0)); }   // _isMute = false, cnt = 0
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;   // (the reference divides by zero here)
        const int n = frames * S;
        SDRGPU_CHECK(part.ensure(sizeof(float) * (size_t)((frames + BANK_F - 1) / BANK_F) * S));
        hipLaunchKernelGGL(bank_squelch_partial_kernel, tiles_by_waves(frames, S), dim3(BANK_W), 0, s, (const float2*)in, frames, S,
                           part.as<float>());
        hipLaunchKernelGGL(bank_squelch_decide_kernel, waves_of(S), dim3(BANK_W), 0, s, part.as<float>(), frames, S, level,
                           state.as<int>());
        hipLaunchKernelGGL(bank_squelch_gate_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const float2*)in, (float2*)out, n, S,
                           state.as<int>());
        SDRGPU_HIP(hipGetLastError());
        return frames;
    }
};

// ------------------------------------------------------------------- magnitude
struct BankMag : Bank {
    int configure(int streams) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        S = streams;
        in_dtype = SDRGPU_C64;
        out_dtype = SDRGPU_F32;
        return SDRGPU_OK;
    }
    int init() override { return SDRGPU_OK; }
    int reset() override { return SDRGPU_OK; }
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        const int n = frames * S;
        hipLaunchKernelGGL(bank_magnitude_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const float2*)in, (float*)out, n);
        SDRGPU_HIP(hipGetLastError());
        return frames;
    }
};

// ---------------------------------------------------------------------- xlator
// channel::FrequencyXlator per stream with the single-stream block's NCO (blocks.h): one offset and one
// running phase for the bank. `real`: the real part only (C64 -> F32), the first stage of BankSSB / BankCW.
struct BankXlator : Bank {
    double w = 0.0;
    bool real = false;
    Nco* nco = nullptr;
    ~BankXlator() override { nco_delete(nco); }
    int configure(int streams, double offsetRad, bool real_) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        if (!std::isfinite(offsetRad)) { set_error("bank_xlator: offset %g not finite", offsetRad); return SDRGPU_EARG; }
        S = streams;
        in_dtype = SDRGPU_C64;
        out_dtype = real_ ? SDRGPU_F32 : SDRGPU_C64;
        real = real_;
        w = xlator_effective_omega(offsetRad);
        return SDRGPU_OK;
    }
    int init() override {
        nco = nco_new();
        return nco_set_w(nco, w);
    }
    int reset() override {   // frequency_xlator.h:35-41
        nco_reset(nco);
        return SDRGPU_OK;
    }
    int set_offset(double offsetRad) {   // frequency_xlator.h:25-29: the phase is kept
        if (!std::isfinite(offsetRad)) { set_error("bank_xlator: offset %g not finite", offsetRad); return SDRGPU_EARG; }
        w = xlator_effective_omega(offsetRad);
        return nco_set_w(nco, w);
    }
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        const float2 *phi, *plo;
        SDRGPU_CHECK(nco_prepare(nco, frames, s, &phi, &plo));
        const int chunks = (S + BANK_XS - 1) / BANK_XS;
        const dim3 grid((unsigned)((frames + BANK_XR - 1) / BANK_XR) * chunks);
        if (real) hipLaunchKernelGGL(bank_xlate_kernel<true>, grid, dim3(BANK_XS), 0, s, (const float2*)in, out, frames, S, chunks, phi, plo);
        else hipLaunchKernelGGL(bank_xlate_kernel<false>, grid, dim3(BANK_XS), 0, s, (const float2*)in, out, frames, S, chunks, phi, plo);
        SDRGPU_HIP(hipGetLastError());
        nco_advance(nco, frames);
        return frames;
    }
};

// ------------------------------------------- decimating FIR, polyphase resampler
// multirate::PolyphaseResampler<T> per stream (polyphase_resampler.h:69-99), and with interp = 1
// filter::DecimatingFIR<D, float> (decimating_fir.h:45-68): the host side of PolyBlock (blocks.hip) over rows.
// offset and phase are the bank's, not a stream's: the streams share their parameters and start together.
struct BankRate : Bank {
    int interp = 1, decim = 1, tpp = 1, phase = 0, offset = 0;
    int R = 0;   // output rows per tile of the tiled kernel at most (a call may take fewer: run); 0: the direct kernel
    std::vector<float> taps;
    DevBuf bankDev, hist[2];
    int cur = 0;
    // The form that runs where the tile fits. Measured at 1024 streams x 1024 rows; the other
    // form: SDRGPU_TUNING=1 SDRGPU_BANK_RATE_TILED=0 | 1, read at creation.
    static constexpr bool kTiledDefault = true;
    // Output rows per tile: R rows read ceil((R - 1) decim / interp) + tpp work rows at most, which fit
    // RATE_LDS where (R - 1) decim <= (RATE_LDS / (64 esize) - tpp) interp. 0: no tile (the direct kernel).
    static int rate_tile_rows(int dtype, int ip, int dc, int tpp_) {
        const long long room = RATE_LDS / (RATE_W * (long long)esize(dtype)) - tpp_;
        if (room < 0) return 0;
        const long long r = std::min<long long>(room * ip / dc + 1, RATE_RMAX);
        return r < RATE_RMIN ? 0 : (int)r;
    }
    int configure(int streams, int dtype, int ip, int dc, const float* t, int ntaps) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        if (!real_or_complex(dtype) || !t || ntaps < 1 || ip < 1 || dc < 1) {
            set_error("bank resampler: dtype %d not F32 / C64, no taps (%d), or interp %d / decim %d below 1", dtype, ntaps, ip, dc);
            return SDRGPU_EARG;
        }
        const long long per = ((long long)ntaps + ip - 1) / ip;
        if ((per - 1) * streams > INT_MAX || per * ip > INT_MAX) {
            set_error("bank resampler: %lld taps per phase of %d phases and %d streams beyond the int index", per, ip, streams);
            return SDRGPU_EARG;
        }
        S = streams;
        in_dtype = out_dtype = dtype;
        interp = ip;
        decim = dc;
        tpp = (int)per;
        taps.assign(t, t + ntaps);
        bool tiled = kTiledDefault;
        if (const char* e = tuning_env("SDRGPU_BANK_RATE_TILED")) tiled = atoi(e) != 0;
        R = tiled ? rate_tile_rows(dtype, ip, dc, tpp) : 0;
        return SDRGPU_OK;
    }
    int HS() const { return (tpp - 1) * S; }
    int init() override {
        // multirate/polyphase_bank.h:15-47: phases[P - 1 - (i % P)][i / P] = taps[i], zero-padded
        std::vector<float> b((size_t)interp * tpp, 0.0f);
        for (size_t i = 0; i < taps.size(); i++) b[(size_t)((interp - 1) - (int)(i % interp)) * tpp + i / interp] = taps[i];
        SDRGPU_CHECK(upload(bankDev, b));
        for (auto& h : hist) SDRGPU_CHECK(h.ensure(esize(in_dtype) * (size_t)std::max(HS(), 1)));
        return reset();
    }
    int reset() override {
        SDRGPU_HIP(hipMemset(hist[cur].p, 0, hist[cur].bytes));
        phase = offset = 0;
        return SDRGPU_OK;
    }
    // while (offset < frames) { out; phase += decim; offset += phase / interp; phase %= interp; }
    long long out_rows(int frames) const override {
        const long long pos = (long long)offset * interp + phase, lim = (long long)frames * interp;
        return pos >= lim ? 0 : (lim - 1 - pos) / decim + 1;
    }
    template <typename DT>
    void launch(const void* in, void* out, const RateArgs& a, hipStream_t s) {
        if (R > 0) {
            const int rowsMost = (int)(((long long)(a.R - 1) * decim + interp - 1) / interp) + tpp;
            const dim3 grid((unsigned)((a.M + a.R - 1) / a.R) * a.chunks);
            hipLaunchKernelGGL(bank_rate_tiled_kernel<DT>, grid, dim3(RATE_TW * RATE_W), sizeof(DT) * (size_t)rowsMost * RATE_W, s,
                               hist[cur].as<DT>(), (const DT*)in, bankDev.as<float>(), (DT*)out, a);
        } else {
            hipLaunchKernelGGL(bank_rate_direct_kernel<DT>, dim3((unsigned)a.M * a.chunks), dim3(RATE_XS), 0, s, hist[cur].as<DT>(),
                               (const DT*)in, bankDev.as<float>(), (DT*)out, a);
        }
    }
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        const int M = (int)out_rows(frames);
        const long long pos0 = (long long)offset * interp + phase;
        if (M > 0) {
            RateArgs a{};
            a.S = S; a.H = tpp - 1; a.tpp = tpp; a.interp = interp;
            a.qD = decim / interp; a.rD = decim % interp;
            a.off0 = offset; a.ph0 = phase;
            a.M = M;
            a.chunks = R > 0 ? (S + RATE_W - 1) / RATE_W : (S + RATE_XS - 1) / RATE_XS;
            // a short call gets smaller tiles, RATE_WGS workgroups where the rows allow, a row per wave at least
            a.R = R > 0 ? std::min<long long>(R, std::max<long long>(RATE_TW, ((long long)M * a.chunks + RATE_WGS - 1) / RATE_WGS)) : 0;
            if (in_dtype == SDRGPU_C64) launch<float2>(in, out, a, s);
            else launch<float>(in, out, a, s);
            SDRGPU_HIP(hipGetLastError());
        }
        if (HS() > 0) {
            SDRGPU_CHECK(carry_history(in_dtype, nullptr, hist[cur], in, hist[cur ^ 1], HS(), frames * S, s));
            cur ^= 1;
        }
        const long long pos = pos0 + (long long)M * decim;
        offset = (int)(pos / interp - frames);
        phase = (int)(pos % interp);
        return M;
    }
};

// the rows as they are: PowerDecimator with a ratio of 1 (power_decimator.h:52-56), RationalResampler's mode 3
struct BankCopy : Bank {
    int configure(int streams, int dtype) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        if (!real_or_complex(dtype)) { set_error("bank copy: dtype %d not F32 / C64", dtype); return SDRGPU_EARG; }
        S = streams;
        in_dtype = out_dtype = dtype;
        return SDRGPU_OK;
    }
    int init() override { return SDRGPU_OK; }
    int reset() override { return SDRGPU_OK; }
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        SDRGPU_HIP(hipMemcpyAsync(out, in, (size_t)frames * S * esize(in_dtype), hipMemcpyDeviceToDevice, s));
        return frames;
    }
};

// ------------------------------------------------------- complex-tap FIR
// filter::FIR<complex_t, complex_t> per stream (fir.h:75): (re, im) tap pairs shared by all streams, F32
// (convert::RealToComplex first, in the same launch) or C64 in, C64 out; `phase`: atan2f of the output
// instead (F32), the stereo decoder's first launch. The kernels and their two forms: bank_wfm_kernels.h.
struct BankCfir : Bank {
    std::vector<float2> taps;
    DevBuf tapsDev, hist[2];
    int cur = 0;
    bool tiled = true, phase = false;
    // The form that runs from CFIR_RMIN rows on. Measured at 1024 streams x 1024 rows, 305 taps;
    // the other form: SDRGPU_TUNING=1 SDRGPU_BANK_CFIR_TILED=0 | 1, read at creation.
    static constexpr bool kTiledDefault = true;
    int configure(int streams, int dtype, const float* t, int ntaps, bool phaseOut) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        if (!real_or_complex(dtype) || !t || ntaps < 1 || (long long)(ntaps - 1) * streams > INT_MAX) {
            set_error("bank_fir_complex: dtype %d not F32 / C64, no taps, or %d taps of %d streams beyond the int index", dtype, ntaps,
                      streams);
            return SDRGPU_EARG;
        }
        S = streams;
        in_dtype = dtype;
        out_dtype = phaseOut ? SDRGPU_F32 : SDRGPU_C64;
        phase = phaseOut;
        taps.resize(ntaps);
        for (int i = 0; i < ntaps; i++) taps[i] = make_float2(t[2 * i], t[2 * i + 1]);
        tiled = kTiledDefault;
        if (const char* e = tuning_env("SDRGPU_BANK_CFIR_TILED")) tiled = atoi(e) != 0;
        return SDRGPU_OK;
    }
    int T() const { return (int)taps.size(); }
    int HS() const { return (T() - 1) * S; }
    int init() override {
        SDRGPU_CHECK(upload(tapsDev, taps));
        for (auto& b : hist) SDRGPU_CHECK(b.ensure(esize(in_dtype) * (size_t)std::max(HS(), 1)));
        return reset();
    }
    int reset() override {
        SDRGPU_HIP(hipMemset(hist[cur].p, 0, hist[cur].bytes));
        return SDRGPU_OK;
    }
    // The tile of a call of M rows: R rows, as many as give CFIR_WGS workgroups, a row per wave at least and
    // CFIR_RPW at most; the taps in the fewest equal segments whose R + Tc - 1 staged rows fit CFIR_LDS.
    void cfir_tile(CfirArgs& a) const {
        a.chunks = (S + CFIR_W - 1) / CFIR_W;
        a.R = (int)std::min<long long>(CFIR_TW * CFIR_RPW, std::max<long long>(CFIR_TW, ((long long)a.M * a.chunks + CFIR_WGS - 1) / CFIR_WGS));
        const int most = CFIR_LDS / (CFIR_W * (int)esize(in_dtype)) - a.R + 1;   // >= 65 taps
        const int segs = (a.T + most - 1) / most;
        a.Tc = (a.T + segs - 1) / segs;
    }
    template <typename IN, bool PHASE>
    void launch(const void* in, void* out, CfirArgs& a, hipStream_t s) {
        if (tiled && a.M >= CFIR_RMIN) {
            cfir_tile(a);
            const dim3 grid((unsigned)((a.M + a.R - 1) / a.R) * a.chunks);
            hipLaunchKernelGGL((bank_cfir_tiled_kernel<IN, PHASE>), grid, dim3(CFIR_TW * CFIR_W), sizeof(IN) * (size_t)(a.R + a.Tc - 1) * CFIR_W,
                               s, hist[cur].as<IN>(), (const IN*)in, tapsDev.as<float2>(), out, a);
        } else {
            a.chunks = (S + CFIR_XS - 1) / CFIR_XS;
            hipLaunchKernelGGL((bank_cfir_direct_kernel<IN, PHASE>), dim3((unsigned)a.M * a.chunks), dim3(CFIR_XS), 0, s, hist[cur].as<IN>(),
                               (const IN*)in, tapsDev.as<float2>(), out, a);
        }
    }
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        CfirArgs a{};
        a.S = S; a.H = T() - 1; a.T = T(); a.M = frames;
        if (in_dtype == SDRGPU_C64) {
            if (phase) launch<float2, true>(in, out, a, s);
            else launch<float2, false>(in, out, a, s);
        } else {
            if (phase) launch<float, true>(in, out, a, s);
            else launch<float, false>(in, out, a, s);
        }
        SDRGPU_HIP(hipGetLastError());
        if (HS() > 0) {
            SDRGPU_CHECK(carry_history(in_dtype, nullptr, hist[cur], in, hist[cur ^ 1], HS(), frames * S, s));
            cur ^= 1;
        }
        return frames;
    }
};

// ------------------------------------------------------------- stereo decoder
// The part of BroadcastFM::process between the quadrature and the audio filters (broadcast_fm.h:147-162, 173-190)
// per stream, with the constants of BroadcastFmBlock::setup (loops.hip): F32 MPX -> C64 (l, r). Three launches:
// the pilot filter on the real MPX writing the pilot's phase, the PLL walk in place on that plane, the matrix.
struct BankStereoDec : Bank {
    BankCfir pilot;
    PllParams pp{};
    float initFreq = 0.0f;
    int delay = 0;             // lprDelay / lmrDelay: the pilot filter's group delay, in rows
    DevBuf pll, hist[2], ph;   // phase[S], freq[S]; the delay line's last `delay` MPX rows, ping-pong; a call's phase plane
    int cur = 0;
    int configure(int streams, double samplerate) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        if (!(samplerate > 0)) { set_error("bank_stereo_decoder: samplerate %g not positive", samplerate); return SDRGPU_EARG; }
        const int np = taps_band_pass_c(18750.0, 19250.0, 3000.0, samplerate, 1, nullptr);
        if (np < 1) return np < 0 ? np : SDRGPU_EARG;
        if ((long long)(np - 1) * streams > INT_MAX) {
            set_error("bank_stereo_decoder: %d pilot taps of %d streams beyond the int index", np, streams);
            return SDRGPU_EARG;
        }
        std::vector<float> pt(2 * (size_t)np);
        taps_band_pass_c(18750.0, 19250.0, 3000.0, samplerate, 1, pt.data());
        SDRGPU_CHECK(pilot.configure(streams, SDRGPU_F32, pt.data(), np, true));
        S = streams;
        in_dtype = SDRGPU_F32;
        out_dtype = SDRGPU_C64;
        delay = ((np - 1) / 2) + 1;
        // PLL(25000 / fs, 0, 19 kHz, 18.75 kHz, 19.25 kHz) (broadcast_fm.h:47)
        critically_damped(25000.0 / samplerate, &pp.alpha, &pp.beta);
        pp.minPhase = -3.1415926535f;
        pp.maxPhase = 3.1415926535f;
        pp.phaseDelta = pp.maxPhase - pp.minPhase;
        pp.minFreq = (float)hz_to_rads(18750.0, samplerate);
        pp.maxFreq = (float)hz_to_rads(19250.0, samplerate);
        initFreq = (float)hz_to_rads(19000.0, samplerate);
        return SDRGPU_OK;
    }
    int DS() const { return delay * S; }   // (delay <= the pilot's history rows, whose product with S fits)
    int init() override {
        pilot.device = device;
        SDRGPU_CHECK(pilot.init());
        for (auto& b : hist) SDRGPU_CHECK(b.ensure(sizeof(float) * (size_t)DS()));
        return reset_own();
    }
    int reset_own() {   // broadcast_fm.h:129-141: the delay lines; the PLL back to (0, 19 kHz)
        SDRGPU_HIP(hipMemset(hist[cur].p, 0, hist[cur].bytes));
        std::vector<float> st(2 * (size_t)S, 0.0f);
        std::fill(st.begin() + S, st.end(), initFreq);
        return upload(pll, st);
    }
    int reset() override {
        SDRGPU_CHECK(pilot.reset());
        return reset_own();
    }
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        const int n = frames * S;
        SDRGPU_CHECK(ph.ensure(sizeof(float) * (size_t)n));
        SDRGPU_CHECK(pilot.run(in, frames, ph.p, s));
        hipLaunchKernelGGL(bank_pll_kernel, waves_of(S), dim3(BANK_W), 0, s, ph.as<float>(), frames, S, pp, pll.as<float>());
        hipLaunchKernelGGL(bank_stereo_matrix_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const float*)in, hist[cur].as<float>(), DS(),
                           ph.as<float>(), (float2*)out, n);
        SDRGPU_HIP(hipGetLastError());
        SDRGPU_CHECK(carry_history(SDRGPU_F32, nullptr, hist[cur], in, hist[cur ^ 1], DS(), n, s));
        cur ^= 1;
        return frames;
    }
};

// convert::MonoToStereo per stream (broadcast_fm.h:211): F32 -> C64 (l, r), l = r
struct BankMonoPairs : Bank {
    int configure(int streams) {
        if (!streams_ok(streams)) return SDRGPU_EARG;
        S = streams;
        in_dtype = SDRGPU_F32;
        out_dtype = SDRGPU_C64;
        return SDRGPU_OK;
    }
    int init() override { return SDRGPU_OK; }
    int reset() override { return SDRGPU_OK; }
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        if (frames == 0) return 0;
        const int n = frames * S;
        hipLaunchKernelGGL(bank_mono_pairs_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const float*)in, (float2*)out, n);
        SDRGPU_HIP(hipGetLastError());
        return frames;
    }
};

// ------------------------------------------------- composites: stages back to back
// Every stage runs on the caller's stream; the stages' rows go through two ping-pong buffers (sized
// for C64) of the largest row count that a stage but the last writes (a resampler may write more rows than
// it reads), which grow on demand.
struct BankChain : Bank {
    std::vector<std::unique_ptr<Bank>> kids;
    DevBuf buf[2];
    size_t keepOnReset = 0;   // the last stages that reset() leaves as they are (AM's low-pass, am.h:104-112)
    // a configured stage joins (rc: its configure's status)
    int add(Bank* b, int rc) {
        std::unique_ptr<Bank> k(b);
        if (rc < 0) return rc;
        kids.push_back(std::move(k));
        return SDRGPU_OK;
    }
    int init() override {   // (add() ran before the create function knew the device: the kids learn it here)
        for (auto& k : kids) {
            k->device = device;
            SDRGPU_CHECK(k->init());
        }
        return SDRGPU_OK;
    }
    int reset() override {
        for (size_t i = 0; i + keepOnReset < kids.size(); i++) SDRGPU_CHECK(kids[i]->reset());
        return SDRGPU_OK;
    }
    bool ragged() const override { return kids.back()->ragged(); }
    void counts(int* c) const override { kids.back()->counts(c); }
    // the rows of the last stage; *most (if given): the largest count a stage before it writes. A stage's
    // count past the index limit ends the walk: the limit + 1 is returned (frames_ok refuses it).
    long long walk_rows(int frames, long long* most) const {
        long long rows = frames, m = 0;
        for (size_t i = 0; i < kids.size(); i++) {
            rows = kids[i]->out_rows((int)rows);
            if (rows > rows_limit()) return rows_limit() + 1;
            if (i + 1 < kids.size()) m = std::max(m, rows);
        }
        if (most) *most = m;
        return rows;
    }
    long long out_rows(int frames) const override { return walk_rows(frames, nullptr); }
    int run(const void* in, int frames, void* out, hipStream_t s) override {
        long long most = 0;
        (void)walk_rows(frames, &most);
        if (kids.size() > 1)
            for (auto& b : buf) SDRGPU_CHECK(b.ensure((size_t)std::max<long long>(most, 1) * S * esize(SDRGPU_C64)));
        const void* cur = in;
        int rows = frames;
        for (size_t i = 0; i < kids.size(); i++) {
            void* dst = i + 1 == kids.size() ? out : buf[i & 1].p;
            rows = kids[i]->run(cur, rows, dst, s);
            if (rows < 0) return rows;
            kids[i]->lastRows = rows;
            cur = dst;
        }
        return rows;
    }
};

// FIR<T, float>(rootRaisedCosine<float>(count, beta, symbolrate, samplerate)) (psk.h:31-32, gfsk.h:32-33)
static int configure_rrc(BankFir* f, int streams, int dtype, int count, double beta, double symbolrate, double samplerate) {
    std::vector<float> t;
    SDRGPU_CHECK(design_taps(t, taps_root_raised_cosine, count, beta, samplerate / symbolrate));
    return f->configure(streams, dtype, t.data(), (int)t.size());
}

}  // namespace sdrgpu

struct sdrgpu_bank {
    sdrgpu::Bank* impl;
};

using namespace sdrgpu;

// The one way a create function hands a new bank to its caller: rc is the status of configure (every
// argument check, nothing on the device yet); then the device, the handle's stream and the device
// state, and the synchronise that publish_block (blocks.h) explains.
static int publish_bank(sdrgpu_bank** h, Bank* b, int device, int rc) {
    std::unique_ptr<Bank> own(b);
    if (rc < 0) return rc;
    b->device = device;
    SDRGPU_SET_DEVICE(device);
    SDRGPU_HIP(hipStreamCreateWithFlags(&b->own, hipStreamNonBlocking));
    SDRGPU_CHECK(b->init());
    SDRGPU_HIP(hipDeviceSynchronize());
    *h = new sdrgpu_bank{own.release()};
    return SDRGPU_OK;
}

#define NEED_BANK(h) do { if (!(h) || !(h)->impl) { set_error("null bank handle"); return SDRGPU_EARG; } } while (0)
#define NEED_BANK_OUT(h, what) do { if (!(h)) { set_error(what ": null handle pointer"); return SDRGPU_EARG; } } while (0)

// ------------------------------------------------------------------- C ABI
extern "C" int sdrgpu_bank_quadrature_create(sdrgpu_bank** h, int device, int streams, double deviationRad) {
    NEED_BANK_OUT(h, "bank_quadrature_create");
    auto* q = new BankQuad();
    return publish_bank(h, q, device, q->configure(streams, deviationRad));
}
extern "C" int sdrgpu_bank_fir_create(sdrgpu_bank** h, int device, int streams, int dtype, const float* taps, int ntaps) {
    NEED_BANK_OUT(h, "bank_fir_create");
    auto* f = new BankFir();
    return publish_bank(h, f, device, f->configure(streams, dtype, taps, ntaps));
}
extern "C" int sdrgpu_bank_fast_agc_create(sdrgpu_bank** h, int device, int streams, int dtype, double setPoint, double maxGain,
                                           double rate, double initGain) {
    NEED_BANK_OUT(h, "bank_fast_agc_create");
    auto* a = new BankFastAgc();
    return publish_bank(h, a, device, a->configure(streams, dtype, setPoint, maxGain, rate, initGain));
}
extern "C" int sdrgpu_bank_costas_create(sdrgpu_bank** h, int device, int streams, int order, double bandwidth, double initPhase,
                                         double initFreq, double minFreq, double maxFreq) {
    NEED_BANK_OUT(h, "bank_costas_create");
    auto* c = new BankCostas();
    return publish_bank(h, c, device, c->configure(streams, order, bandwidth, initPhase, initFreq, minFreq, maxFreq));
}
extern "C" int sdrgpu_bank_mm_create(sdrgpu_bank** h, int device, int streams, int dtype, double omega, double omegaGain,
                                     double muGain, double omegaRelLimit, int interpPhases, int interpTaps) {
    NEED_BANK_OUT(h, "bank_mm_create");
    auto* m = new BankMm();
    return publish_bank(h, m, device, m->configure(streams, dtype, omega, omegaGain, muGain, omegaRelLimit, interpPhases, interpTaps));
}

// the stages and constants of sdrgpu_psk_create (symsync.hip)
extern "C" int sdrgpu_bank_psk_create(sdrgpu_bank** h, int device, int streams, int order, double symbolrate, double samplerate,
                                      int rrcTapCount, double rrcBeta, double agcRate, double costasBandwidth, double omegaGain,
                                      double muGain, double omegaRelLimit) {
    NEED_BANK_OUT(h, "bank_psk_create");
    auto* c = new BankChain();
    int rc = SDRGPU_OK;
    if (!Bank::streams_ok(streams)) rc = SDRGPU_EARG;
    else if (!(symbolrate > 0) || !(samplerate > 0)) { set_error("bank_psk_create: bad argument"); rc = SDRGPU_EARG; }
    c->S = std::max(streams, 1);
    c->in_dtype = c->out_dtype = SDRGPU_C64;
    if (rc >= 0) { auto* f = new BankFir(); rc = c->add(f, configure_rrc(f, streams, SDRGPU_C64, rrcTapCount, rrcBeta, symbolrate, samplerate)); }
    if (rc >= 0) { auto* a = new BankFastAgc(); rc = c->add(a, a->configure(streams, SDRGPU_C64, 1.0, 10e6, agcRate, 1.0)); }
    const double PI = 3.1415926535f;   // FL_M_PI, the default frequency limits (pll.h:15)
    if (rc >= 0) { auto* l = new BankCostas(); rc = c->add(l, l->configure(streams, order, costasBandwidth, 0.0, 0.0, -PI, PI)); }
    if (rc >= 0) {
        auto* m = new BankMm();
        rc = c->add(m, m->configure(streams, SDRGPU_C64, samplerate / symbolrate, omegaGain, muGain, omegaRelLimit, 128, 8));
    }
    return publish_bank(h, c, device, rc);
}

extern "C" int sdrgpu_bank_pll_create(sdrgpu_bank** h, int device, int streams, double bandwidth, double initPhase, double initFreq,
                                      double minFreq, double maxFreq) {
    NEED_BANK_OUT(h, "bank_pll_create");
    auto* c = new BankPll();
    return publish_bank(h, c, device, c->configure(streams, PllKind::Pll, bandwidth, 0, 0, initPhase, initFreq, minFreq, maxFreq));
}
extern "C" int sdrgpu_bank_carrier_pll_create(sdrgpu_bank** h, int device, int streams, double bandwidth, double initPhase,
                                              double initFreq, double minFreq, double maxFreq) {
    NEED_BANK_OUT(h, "bank_carrier_pll_create");
    auto* c = new BankPll();
    return publish_bank(h, c, device, c->configure(streams, PllKind::Carrier, bandwidth, 0, 0, initPhase, initFreq, minFreq, maxFreq));
}
extern "C" int sdrgpu_bank_meteor_costas_create(sdrgpu_bank** h, int device, int streams, double bandwidth, int brokenModulation,
                                                double initPhase, double initFreq, double minFreq, double maxFreq) {
    NEED_BANK_OUT(h, "bank_meteor_costas_create");
    auto* c = new BankPll();
    return publish_bank(h, c, device,
                        c->configure(streams, PllKind::Meteor, bandwidth, brokenModulation, 0, initPhase, initFreq, minFreq, maxFreq));
}

// the stages and constants of sdrgpu_meteor_create (symsync.hip)
extern "C" int sdrgpu_bank_meteor_create(sdrgpu_bank** h, int device, int streams, double symbolrate, double samplerate,
                                         int rrcTapCount, double rrcBeta, double agcRate, double costasBandwidth,
                                         int brokenModulation, int oqpsk, double omegaGain, double muGain, double omegaRelLimit) {
    NEED_BANK_OUT(h, "bank_meteor_create");
    auto* c = new BankChain();
    int rc = SDRGPU_OK;
    if (!Bank::streams_ok(streams)) rc = SDRGPU_EARG;
    else if (!(symbolrate > 0) || !(samplerate > 0)) { set_error("bank_meteor_create: bad argument"); rc = SDRGPU_EARG; }
    c->S = std::max(streams, 1);
    c->in_dtype = c->out_dtype = SDRGPU_C64;
    if (rc >= 0) { auto* f = new BankFir(); rc = c->add(f, configure_rrc(f, streams, SDRGPU_C64, rrcTapCount, rrcBeta, symbolrate, samplerate)); }
    if (rc >= 0) { auto* a = new BankFastAgc(); rc = c->add(a, a->configure(streams, SDRGPU_C64, 1.0, 10e6, agcRate, 1.0)); }
    const double PI = 3.1415926535f;   // FL_M_PI, the default frequency limits (meteor_costas.h:13)
    if (rc >= 0) {
        auto* l = new BankPll();
        rc = c->add(l, l->configure(streams, PllKind::Meteor, costasBandwidth, brokenModulation, oqpsk, 0.0, 0.0, -PI, PI));
    }
    if (rc >= 0) {
        auto* m = new BankMm();
        rc = c->add(m, m->configure(streams, SDRGPU_C64, samplerate / symbolrate, omegaGain, muGain, omegaRelLimit, 128, 8));
    }
    return publish_bank(h, c, device, rc);
}

// the stages and constants of sdrgpu_gfsk_create (symsync.hip)
extern "C" int sdrgpu_bank_gfsk_create(sdrgpu_bank** h, int device, int streams, double symbolrate, double samplerate, double deviation,
                                       int rrcTapCount, double rrcBeta, double omegaGain, double muGain, double omegaRelLimit) {
    NEED_BANK_OUT(h, "bank_gfsk_create");
    auto* c = new BankChain();
    int rc = SDRGPU_OK;
    if (!Bank::streams_ok(streams)) rc = SDRGPU_EARG;
    else if (!(symbolrate > 0) || !(samplerate > 0)) { set_error("bank_gfsk_create: bad argument"); rc = SDRGPU_EARG; }
    c->S = std::max(streams, 1);
    c->in_dtype = SDRGPU_C64;
    c->out_dtype = SDRGPU_F32;
    if (rc >= 0) { auto* q = new BankQuad(); rc = c->add(q, q->configure(streams, hz_to_rads(deviation, samplerate))); }
    if (rc >= 0) { auto* f = new BankFir(); rc = c->add(f, configure_rrc(f, streams, SDRGPU_F32, rrcTapCount, rrcBeta, symbolrate, samplerate)); }
    if (rc >= 0) {
        auto* m = new BankMm();
        rc = c->add(m, m->configure(streams, SDRGPU_F32, samplerate / symbolrate, omegaGain, muGain, omegaRelLimit, 128, 8));
    }
    return publish_bank(h, c, device, rc);
}

// loop::AGC<T> per stream (agc.h:13-147)
extern "C" int sdrgpu_bank_agc_create(sdrgpu_bank** h, int device, int streams, int dtype, double setPoint, double attack, double decay,
                                      double maxGain, double maxOutputAmp, double initGain, int enabled) {
    NEED_BANK_OUT(h, "bank_agc_create");
    auto* a = new BankAgc();
    return publish_bank(h, a, device, a->configure(streams, dtype, setPoint, attack, decay, maxGain, maxOutputAmp, initGain, enabled));
}
// AGC::setGain (agc.h:31-35) for every stream: of an AGC bank, or of the last AGC of a chain (BankAM's
// audio AGC, as sdrgpu_demod_agc_set_gain(h, 1, gain))
extern "C" int sdrgpu_bank_agc_set_gain(sdrgpu_bank* h, float gain) {
    NEED_BANK(h);
    auto* a = dynamic_cast<BankAgc*>(h->impl);
    if (auto* c = dynamic_cast<BankChain*>(h->impl))
        for (auto& k : c->kids)
            if (auto* ka = dynamic_cast<BankAgc*>(k.get())) a = ka;
    if (!a) { set_error("bank_agc_set_gain: the bank has no AGC"); return SDRGPU_ESTATE; }
    a->set_gain(gain);
    return SDRGPU_OK;
}
// correction::DCBlocker<T> per stream (dc_blocker.h:54-60)
extern "C" int sdrgpu_bank_dc_blocker_create(sdrgpu_bank** h, int device, int streams, int dtype, double rate) {
    NEED_BANK_OUT(h, "bank_dc_blocker_create");
    auto* d = new BankDcb();
    return publish_bank(h, d, device, d->configure(streams, dtype, rate));
}
// filter::Deemphasis<float> per stream (deephasis.h:58-65, 91-94)
extern "C" int sdrgpu_bank_deemphasis_create(sdrgpu_bank** h, int device, int streams, double tau, double samplerate) {
    NEED_BANK_OUT(h, "bank_deemphasis_create");
    auto* d = new BankDeemp();
    return publish_bank(h, d, device, d->configure(streams, tau, samplerate, false));
}
// filter::Deemphasis<stereo_t> per stream (deephasis.h:67-77): C64 rows of (l, r)
extern "C" int sdrgpu_bank_deemphasis_stereo_create(sdrgpu_bank** h, int device, int streams, double tau, double samplerate) {
    NEED_BANK_OUT(h, "bank_deemphasis_stereo_create");
    auto* d = new BankDeemp();
    return publish_bank(h, d, device, d->configure(streams, tau, samplerate, true));
}
// noise_reduction::Squelch per stream (squelch.h:33-63)
extern "C" int sdrgpu_bank_squelch_create(sdrgpu_bank** h, int device, int streams, double level) {
    NEED_BANK_OUT(h, "bank_squelch_create");
    auto* q = new BankSquelch();
    return publish_bank(h, q, device, q->configure(streams, level));
}
extern "C" int sdrgpu_bank_squelch_muted(sdrgpu_bank* h, int* muted) {
    NEED_BANK(h);
    auto* q = dynamic_cast<BankSquelch*>(h->impl);
    if (!q || !muted) { set_error("bank_squelch_muted: not a squelch bank, or a null pointer"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(q->device);
    SDRGPU_HIP(hipDeviceSynchronize());   // (UI-rate query: waits for the bank's queued work)
    SDRGPU_HIP(hipMemcpy(muted, q->state.p, sizeof(int) * q->S, hipMemcpyDeviceToHost));
    return SDRGPU_OK;
}

// a chain of C64 in, F32 out; rc: the status of the checks so far
static BankChain* new_audio_chain(int streams, int& rc) {
    auto* c = new BankChain();
    if (!Bank::streams_ok(streams)) rc = SDRGPU_EARG;
    c->S = std::max(streams, 1);
    c->in_dtype = SDRGPU_C64;
    c->out_dtype = SDRGPU_F32;
    return c;
}

// demod::FM<float> per stream (fm.h:25-44, 86-93, 117-145): the stages and taps of sdrgpu_fm_create (blocks.hip)
extern "C" int sdrgpu_bank_fm_create(sdrgpu_bank** h, int device, int streams, double samplerate, double bandwidth, int lowPass,
                                     int highPass) {
    NEED_BANK_OUT(h, "bank_fm_create");
    int rc = SDRGPU_OK;
    auto* c = new_audio_chain(streams, rc);
    if (rc >= 0 && (!(samplerate > 0) || !(bandwidth > 0))) { set_error("bank_fm_create: samplerate and bandwidth must be positive"); rc = SDRGPU_EARG; }
    if (rc >= 0) { auto* q = new BankQuad(); rc = c->add(q, q->configure(streams, hz_to_rads(bandwidth / 2.0, samplerate))); }
    if (rc >= 0 && (lowPass || highPass)) {
        std::vector<float> t;
        rc = (lowPass && highPass) ? design_taps(t, taps_band_pass_f, 300.0, bandwidth / 2.0, 100.0, samplerate, 0)
             : highPass            ? design_taps(t, taps_high_pass, 300.0, 100.0, samplerate, 0)
                                   : design_taps(t, taps_low_pass, bandwidth / 2.0, (bandwidth / 2.0) * 0.1, samplerate, 0);
        if (rc >= 0) { auto* f = new BankFir(); rc = c->add(f, f->configure(streams, SDRGPU_F32, t.data(), (int)t.size())); }
    }
    return publish_bank(h, c, device, rc);
}

// demod::AM<float> per stream (am.h:28-49, 114-131): the stages and constants of sdrgpu_am_create (loops.hip), mono
extern "C" int sdrgpu_bank_am_create(sdrgpu_bank** h, int device, int streams, int agcMode, double bandwidth, double agcAttack,
                                     double agcDecay, double dcBlockRate, double samplerate) {
    NEED_BANK_OUT(h, "bank_am_create");
    int rc = SDRGPU_OK;
    auto* c = new_audio_chain(streams, rc);
    if (rc >= 0 && (agcMode < 0 || agcMode > 2 || !(samplerate > 0) || !(bandwidth > 0))) {
        set_error("bank_am_create: agcMode %d outside 0..2, or samplerate or bandwidth not positive", agcMode);
        rc = SDRGPU_EARG;
    }
    // the AGC of AM (am.h:27-49): set point 1, max gain 10e6, max output 10, initial gain inf
    auto agc = [&](int dtype, int enabled) {
        auto* a = new BankAgc();
        return c->add(a, a->configure(streams, dtype, 1.0, agcAttack, agcDecay, 10e6, 10.0, INFINITY, enabled));
    };
    if (rc >= 0 && agcMode == 1) rc = agc(SDRGPU_C64, 1);
    if (rc >= 0) { auto* m = new BankMag(); rc = c->add(m, m->configure(streams)); }
    if (rc >= 0) { auto* d = new BankDcb(); rc = c->add(d, d->configure(streams, SDRGPU_F32, dcBlockRate)); }
    if (rc >= 0 && agcMode != 1) rc = agc(SDRGPU_F32, agcMode == 2);   // audioAgc runs unless CARRIER; enabled only for AUDIO
    if (rc >= 0) {
        const double fc = bandwidth / 2.0;
        std::vector<float> t;
        rc = design_taps(t, taps_low_pass, fc, fc * 0.1, samplerate, 0);
        if (rc >= 0) { auto* f = new BankFir(); rc = c->add(f, f->configure(streams, SDRGPU_F32, t.data(), (int)t.size())); }
        if (rc >= 0) c->keepOnReset = 1;   // reset() (am.h:104-112): the AGCs and the DC blocker, not lpf
    }
    return publish_bank(h, c, device, rc);
}

// channel::FrequencyXlator per stream (frequency_xlator.h:15-50)
extern "C" int sdrgpu_bank_xlator_create(sdrgpu_bank** h, int device, int streams, double offsetRad) {
    NEED_BANK_OUT(h, "bank_xlator_create");
    auto* x = new BankXlator();
    return publish_bank(h, x, device, x->configure(streams, offsetRad, false));
}
// ... and its real part in the same launch (convert::ComplexToReal after the xlator: ssb.h:92-93, cw.h:73-75), C64 -> F32:
// the first stage of BankSSB / BankCW on its own
extern "C" int sdrgpu_bank_xlator_real_create(sdrgpu_bank** h, int device, int streams, double offsetRad) {
    NEED_BANK_OUT(h, "bank_xlator_real_create");
    auto* x = new BankXlator();
    return publish_bank(h, x, device, x->configure(streams, offsetRad, true));
}
// FrequencyXlator::setOffset (frequency_xlator.h:25-29) of an xlator bank, or of the xlator of a BankSSB / BankCW chain
extern "C" int sdrgpu_bank_xlator_set_offset(sdrgpu_bank* h, double offsetRad) {
    NEED_BANK(h);
    auto* x = dynamic_cast<BankXlator*>(h->impl);
    if (auto* c = dynamic_cast<BankChain*>(h->impl))
        for (auto& k : c->kids)
            if (!x) x = dynamic_cast<BankXlator*>(k.get());
    if (!x) { set_error("bank_xlator_set_offset: the bank has no xlator"); return SDRGPU_ESTATE; }
    if (!std::isfinite(offsetRad)) { set_error("bank_xlator_set_offset: offset %g not finite", offsetRad); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(h->impl->device);   // (the handle's: a chain's xlator runs where the chain does)
    SDRGPU_HIP(hipDeviceSynchronize());   // (a queued call still reads the fine table that the setter rewrites)
    return x->set_offset(offsetRad);
}

// [xlate by offsetRad -> Re] -> bank AGC<F32>(1, attack, decay, 10e6, maxOutputAmp, initGain): the stages of SSB and CW
static int publish_xlate_agc(sdrgpu_bank** h, int device, int streams, int rc, double offsetRad, int agcEnabled, double attack,
                             double decay, double maxOutputAmp, double initGain) {
    auto* c = new_audio_chain(streams, rc);
    if (rc >= 0) { auto* x = new BankXlator(); rc = c->add(x, x->configure(streams, offsetRad, true)); }
    if (rc >= 0) {
        auto* a = new BankAgc();
        rc = c->add(a, a->configure(streams, SDRGPU_F32, 1.0, attack, decay, 10e6, maxOutputAmp, initGain, agcEnabled));
    }
    return publish_bank(h, c, device, rc);
}

// demod::SSB<float> per stream (ssb.h:21-35, 90-105, 119-126): the stages and constants of sdrgpu_ssb_create (loops.hip), mono
extern "C" int sdrgpu_bank_ssb_create(sdrgpu_bank** h, int device, int streams, int mode, double bandwidth, double samplerate,
                                      int agcEnabled, double agcAttack, double agcDecay) {
    NEED_BANK_OUT(h, "bank_ssb_create");
    int rc = SDRGPU_OK;
    if (mode < 0 || mode > 2 || !std::isfinite(bandwidth) || !std::isfinite(samplerate) || !(samplerate > 0)) {
        set_error("bank_ssb_create: mode %d outside 0..2, bandwidth not finite, or samplerate not finite and positive", mode);
        rc = SDRGPU_EARG;
    }
    const double tr = mode == 0 ? bandwidth / 2.0 : (mode == 1 ? -bandwidth / 2.0 : 0.0);   // getTranslation (ssb.h:119-126)
    return publish_xlate_agc(h, device, streams, rc, rc >= 0 ? hz_to_rads(tr, samplerate) : 0.0, agcEnabled, agcAttack, agcDecay, 10.0,
                             INFINITY);
}

// demod::CW<float> per stream (cw.h:15-28, 72-85): the stages and constants of sdrgpu_cw_create (loops.hip), mono
extern "C" int sdrgpu_bank_cw_create(sdrgpu_bank** h, int device, int streams, double tone, int agcEnabled, double agcAttack,
                                     double agcDecay, double samplerate) {
    NEED_BANK_OUT(h, "bank_cw_create");
    int rc = SDRGPU_OK;
    if (!std::isfinite(tone) || !std::isfinite(samplerate) || !(samplerate > 0)) {
        set_error("bank_cw_create: tone not finite, or samplerate not finite and positive");
        rc = SDRGPU_EARG;
    }
    return publish_xlate_agc(h, device, streams, rc, rc >= 0 ? hz_to_rads(tone, samplerate) : 0.0, agcEnabled, agcAttack, agcDecay, 1.0,
                             1.0);
}

// -- rate-changing banks
// filter::DecimatingFIR<D, float> per stream (decimating_fir.h:45-68): the resampler bank with one phase
extern "C" int sdrgpu_bank_decimating_fir_create(sdrgpu_bank** h, int device, int streams, int dtype, const float* taps, int ntaps,
                                                 int decim) {
    NEED_BANK_OUT(h, "bank_decimating_fir_create");
    auto* r = new BankRate();
    return publish_bank(h, r, device, r->configure(streams, dtype, 1, decim, taps, ntaps));
}
// multirate::PolyphaseResampler<T> per stream (polyphase_resampler.h:69-99)
extern "C" int sdrgpu_bank_polyphase_resampler_create(sdrgpu_bank** h, int device, int streams, int dtype, int interp, int decim,
                                                      const float* taps, int ntaps) {
    NEED_BANK_OUT(h, "bank_polyphase_resampler_create");
    auto* r = new BankRate();
    return publish_bank(h, r, device, r->configure(streams, dtype, interp, decim, taps, ntaps));
}

// a chain of one element type; rc: the status of the checks so far
static BankChain* new_rate_chain(int streams, int dtype, int& rc) {
    auto* c = new BankChain();
    if (!Bank::streams_ok(streams)) rc = SDRGPU_EARG;
    else if (!real_or_complex(dtype)) { set_error("bank resampler: dtype %d not F32 / C64", dtype); rc = SDRGPU_EARG; }
    c->S = std::max(streams, 1);
    c->in_dtype = c->out_dtype = dtype;
    return c;
}
static int add_copy(BankChain* c, int streams, int dtype) {
    auto* b = new BankCopy();
    return c->add(b, b->configure(streams, dtype));
}
// multirate::PowerDecimator<T> (power_decimator.h:51-108): the stages of the plan, one decimating FIR bank each
static int add_power_decim(BankChain* c, int streams, int dtype, int ratio) {
    if (ratio == 1) return add_copy(c, streams, dtype);
    int d[8], n[8];
    const float* t[8];
    const int ns = decim_plan(ratio, d, n, t);
    if (ns < 0) return ns;
    for (int i = 0; i < ns; i++) {
        auto* r = new BankRate();
        SDRGPU_CHECK(c->add(r, r->configure(streams, dtype, 1, d[i], t[i], n[i])));
    }
    return SDRGPU_OK;
}
extern "C" int sdrgpu_bank_power_decimator_create(sdrgpu_bank** h, int device, int streams, int dtype, int ratio) {
    NEED_BANK_OUT(h, "bank_power_decimator_create");
    int rc = SDRGPU_OK;
    auto* c = new_rate_chain(streams, dtype, rc);
    if (rc >= 0) rc = add_power_decim(c, streams, dtype, ratio);
    return publish_bank(h, c, device, rc);
}
// multirate::RationalResampler<T> (rational_resampler.h:121-167): the plan of sdrgpu_rational_resampler_create
extern "C" int sdrgpu_bank_rational_resampler_create(sdrgpu_bank** h, int device, int streams, int dtype, double inSamplerate,
                                                     double outSamplerate) {
    NEED_BANK_OUT(h, "bank_rational_resampler_create");
    int rc = SDRGPU_OK;
    auto* c = new_rate_chain(streams, dtype, rc);
    RationalPlan rp;
    if (rc >= 0) rc = plan_rational(inSamplerate, outSamplerate, rp);
    if (rc >= 0 && (rp.mode == 0 || rp.mode == 1)) rc = add_power_decim(c, streams, dtype, rp.predec);
    if (rc >= 0 && (rp.mode == 0 || rp.mode == 2)) {
        auto* r = new BankRate();
        rc = c->add(r, r->configure(streams, dtype, rp.interp, rp.decim, rp.taps.data(), (int)rp.taps.size()));
    }
    if (rc >= 0 && rp.mode == 3) rc = add_copy(c, streams, dtype);
    return publish_bank(h, c, device, rc);
}

// -- broadcast FM
// filter::FIR<complex_t, complex_t> per stream (fir.h:75); in_dtype F32: convert::RealToComplex first, in the same launch
extern "C" int sdrgpu_bank_fir_complex_create(sdrgpu_bank** h, int device, int streams, int in_dtype, const float* taps, int ntaps) {
    NEED_BANK_OUT(h, "bank_fir_complex_create");
    auto* f = new BankCfir();
    return publish_bank(h, f, device, f->configure(streams, in_dtype, taps, ntaps, false));
}
// the stereo decoder of demod::BroadcastFM per stream (broadcast_fm.h:147-162, 173-190): F32 MPX -> C64 (l, r)
extern "C" int sdrgpu_bank_stereo_decoder_create(sdrgpu_bank** h, int device, int streams, double samplerate) {
    NEED_BANK_OUT(h, "bank_stereo_decoder_create");
    auto* d = new BankStereoDec();
    return publish_bank(h, d, device, d->configure(streams, samplerate));
}
// demod::BroadcastFM per stream (broadcast_fm.h:34-60, 144-215): the stages and constants of sdrgpu_broadcast_fm_create
// (loops.hip) without the RDS branch. As there, the audio low-pass is designed whether it runs or not: a
// sample rate at which it has no taps is refused either way.
extern "C" int sdrgpu_bank_broadcast_fm_create(sdrgpu_bank** h, int device, int streams, double deviation, double samplerate,
                                               int stereo, int lowPass) {
    NEED_BANK_OUT(h, "bank_broadcast_fm_create");
    auto* c = new BankChain();
    int rc = SDRGPU_OK;
    if (!Bank::streams_ok(streams)) rc = SDRGPU_EARG;
    else if (!(samplerate > 0) || !(deviation > 0)) { set_error("bank_broadcast_fm_create: samplerate and deviation must be positive"); rc = SDRGPU_EARG; }
    c->S = std::max(streams, 1);
    c->in_dtype = c->out_dtype = SDRGPU_C64;
    std::vector<float> at;
    if (rc >= 0) rc = design_taps(at, taps_low_pass, 15000.0, 4000.0, samplerate, 0);
    if (rc >= 0) { auto* q = new BankQuad(); rc = c->add(q, q->configure(streams, hz_to_rads(deviation, samplerate))); }
    if (rc >= 0 && stereo) { auto* d = new BankStereoDec(); rc = c->add(d, d->configure(streams, samplerate)); }
    // alFir / arFir (broadcast_fm.h:205-208): the (l, r) pairs as one C64 stream through real taps; mono: the MPX
    if (rc >= 0 && lowPass) { auto* f = new BankFir(); rc = c->add(f, f->configure(streams, stereo ? SDRGPU_C64 : SDRGPU_F32, at.data(), (int)at.size())); }
    if (rc >= 0 && !stereo) { auto* m = new BankMonoPairs(); rc = c->add(m, m->configure(streams)); }
    return publish_bank(h, c, device, rc);
}

extern "C" int sdrgpu_bank_streams(sdrgpu_bank* h) {
    NEED_BANK(h);
    return h->impl->S;
}

extern "C" int sdrgpu_bank_out_rows(sdrgpu_bank* h, int frames) {
    NEED_BANK(h);
    return h->impl->frames_ok(frames) ? (int)h->impl->out_rows(frames) : SDRGPU_EARG;
}

extern "C" int sdrgpu_bank_process_dev(sdrgpu_bank* h, const void* in, int frames, void* out, void* stream) {
    NEED_BANK(h);
    Bank* b = h->impl;
    if (!b->frames_ok(frames)) return SDRGPU_EARG;
    if (frames > 0 && (!in || !out)) { set_error("bank_process: bad buffers"); return SDRGPU_EARG; }
    const hipStream_t s = stream ? (hipStream_t)stream : b->own;
    SDRGPU_SET_DEVICE(b->device);
    SDRGPU_CHECK(b->order.follow(s));
    OrderScope od(b->order, s);
    const int rows = b->run(in, frames, out, s);
    if (rows >= 0) b->lastRows = rows;
    return rows;
}

// Host buffers through the handle's pinned staging. A bank with data-dependent counts leaves the
// elements past a stream's count as they were: its device rows start as a copy of the caller's `out`.
extern "C" int sdrgpu_bank_process(sdrgpu_bank* h, const void* in, int frames, void* out) {
    NEED_BANK(h);
    Bank* b = h->impl;
    if (!b->frames_ok(frames)) return SDRGPU_EARG;
    if (frames > 0 && (!in || !out)) { set_error("bank_process: bad buffers"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(b->device);
    const size_t inB = (size_t)frames * b->S * esize(b->in_dtype);
    const size_t outB = (size_t)b->out_rows(frames) * b->S * esize(b->out_dtype);   // (a resampler may write more rows than it reads)
    SDRGPU_CHECK(b->pin_in.ensure(std::max<size_t>(inB, 1)));
    SDRGPU_CHECK(b->pin_out.ensure(std::max<size_t>(outB, 1)));
    SDRGPU_CHECK(b->dev_in.ensure(std::max<size_t>(inB, 1)));
    SDRGPU_CHECK(b->dev_out.ensure(std::max<size_t>(outB, 1)));
    if (frames > 0) std::memcpy(b->pin_in.p, in, inB);
    if (frames > 0 && b->ragged()) std::memcpy(b->pin_out.p, out, outB);
    SDRGPU_CHECK(b->order.follow(b->own));
    OrderScope od(b->order, b->own);
    if (frames > 0) SDRGPU_HIP(hipMemcpyAsync(b->dev_in.p, b->pin_in.p, inB, hipMemcpyHostToDevice, b->own));
    if (frames > 0 && b->ragged()) SDRGPU_HIP(hipMemcpyAsync(b->dev_out.p, b->pin_out.p, outB, hipMemcpyHostToDevice, b->own));
    const int rows = b->run(b->dev_in.p, frames, b->dev_out.p, b->own);
    if (rows < 0) return rows;
    b->lastRows = rows;
    const size_t gotB = (size_t)rows * b->S * esize(b->out_dtype);
    if (rows > 0) SDRGPU_HIP(hipMemcpyAsync(b->pin_out.p, b->dev_out.p, gotB, hipMemcpyDeviceToHost, b->own));
    SDRGPU_HIP(hipStreamSynchronize(b->own));
    if (rows > 0) std::memcpy(out, b->pin_out.p, gotB);
    return rows;
}

extern "C" int sdrgpu_bank_out_counts(sdrgpu_bank* h, int* counts) {
    NEED_BANK(h);
    if (!counts) { set_error("bank_out_counts: null pointer"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(h->impl->device);
    SDRGPU_HIP(hipDeviceSynchronize());
    h->impl->counts(counts);
    return SDRGPU_OK;
}

extern "C" int sdrgpu_bank_reset(sdrgpu_bank* h) {
    NEED_BANK(h);
    SDRGPU_SET_DEVICE(h->impl->device);
    SDRGPU_HIP(hipDeviceSynchronize());   // (the state a queued call still reads is rewritten on the null stream)
    SDRGPU_CHECK(h->impl->reset());
    h->impl->lastRows = 0;
    SDRGPU_HIP(hipDeviceSynchronize());
    return SDRGPU_OK;
}

extern "C" int sdrgpu_bank_destroy(sdrgpu_bank* h) {
    if (!h) return SDRGPU_OK;
    if (h->impl) {
        (void)hipSetDevice(h->impl->device);
        (void)hipDeviceSynchronize();
        delete h->impl;
    }
    delete h;
    return SDRGPU_OK;
}
