// Host side of the serial loops and of the demodulators composed from them (the kernels are in
// loop_kernels.h, which also says why this file is built with -ffp-contract=off):
//   loop::AGC<T>, correction::DCBlocker, noise_reduction::NoiseBlanker, filter::Deemphasis<T>
//   demod::AM<T>        demod/am.h:114-142     ([carrier AGC] -> |x| -> DC block -> [audio AGC] -> LPF)
//   demod::SSB<T>       demod/ssb.h:90-105     (xlate +-bw/2 -> Re -> AGC)
//   demod::CW<T>        demod/cw.h:72-85       (xlate tone -> Re -> AGC)
//   demod::BroadcastFM  demod/broadcast_fm.h   (stereo decoder and RDS branch)
// Top to bottom: the block structs (each: configuration, state, setup / reset, its launch in run),
// the chain-building helpers, the C entry points. The structs select no device and own no stream: an
// entry point does, through enter_block or, for a create, itself and publish_block (blocks.h, which
// also states when an entry point waits for the device).
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>
#include "sdrgpu_internal.h"
#include "blocks.h"
#include "loop_kernels.h"

namespace sdrgpu {

struct AgcBlock : Block {
    AgcParams p{};
    float initGain = 1.0f;
    DevBuf state, cm, pend;
    bool pending = false;
    float pendingGain = 0.0f;
    // AGC::init and the setters (agc.h:13-26, 44-79): members are float. The running amplitude and
    // gain (device state) are kept.
    void set_attack_decay(double attack, double decay) {
        p.attack = (float)attack;
        p.invAttack = 1.0f - p.attack;
        p.decay = (float)decay;
        p.invDecay = 1.0f - p.decay;
    }
    void set_params(double setPoint, double attack, double decay, double maxGain, double maxOutputAmp, double initGain_) {
        p.setPoint = (float)setPoint;
        set_attack_decay(attack, decay);
        p.maxGain = (float)maxGain;
        p.maxOutputAmp = (float)maxOutputAmp;
        initGain = (float)initGain_;
    }
    int setup(int dev, int dtype, double setPoint, double attack, double decay, double maxGain, double maxOutputAmp,
              double initGain_) {
        device = dev;
        in_dtype = out_dtype = dtype;
        set_params(setPoint, attack, decay, maxGain, maxOutputAmp, initGain_);
        p.enabled = 1;
        SDRGPU_CHECK(state.ensure(sizeof(AgcState)));
        SDRGPU_CHECK(pend.ensure(sizeof(float)));
        return reset();
    }
    int out_count(int count) override { return count; }
    int reset() override {   // agc.h:81-86
        AgcState s;
        s.amp = p.setPoint / initGain;
        s.gain = (p.maxGain < initGain) ? p.maxGain : initGain;
        SDRGPU_HIP(hipMemcpy(state.p, &s, sizeof(s), hipMemcpyHostToDevice));
        pending = false;
        return SDRGPU_OK;
    }
    int set_gain(float g) {   // agc.h:31-35, applied at the next process()
        SDRGPU_HIP(hipMemcpy(pend.p, &g, sizeof(g), hipMemcpyHostToDevice));
        pending = true;
        pendingGain = g;
        return SDRGPU_OK;
    }
    int get_gain(float* gain) {   // (the caller has waited for the block's queued work unless `pending`)
        if (pending) { *gain = pendingGain; return SDRGPU_OK; }
        AgcState s;
        SDRGPU_HIP(hipMemcpy(&s, state.p, sizeof(s), hipMemcpyDeviceToHost));
        *gain = s.gain;
        return SDRGPU_OK;
    }
    template <typename DT>
    void run_t(const void* in, int count, void* out, int nchunks, const float* pg, hipStream_t s) {
        if (count > 0 && p.enabled)
            hipLaunchKernelGGL(chunk_max_kernel<DT>, dim3(nchunks), dim3(LOOP_NT), 0, s, (const DT*)in, count, cm.as<float>());
        hipLaunchKernelGGL(agc_kernel<DT>, dim3(1), dim3(LOOP_NT), 0, s, (const DT*)in, (DT*)out, count, p,
                           state.as<AgcState>(), cm.as<float>(), pg);
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("agc: negative count"); return SDRGPU_EARG; }
        const float* pg = pending ? pend.as<float>() : nullptr;
        pending = false;
        if (count == 0 && !pg) return 0;
        const int nchunks = std::max(1, (count + LOOP_CHUNK - 1) / LOOP_CHUNK);
        SDRGPU_CHECK(cm.ensure(sizeof(float) * nchunks));
        if (in_dtype == SDRGPU_C64) run_t<float2>(in, count, out, nchunks, pg, s);
        else run_t<float>(in, count, out, nchunks, pg, s);
        SDRGPU_HIP(hipGetLastError());
        return count;
    }
};

struct DcbBlock : Block {
    float rate = 0.0f;
    DevBuf state;
    int setup(int dev, int dtype, double r) {
        device = dev;
        in_dtype = out_dtype = dtype;
        rate = (float)r;
        SDRGPU_CHECK(state.ensure(sizeof(float2)));
        return reset();
    }
    int out_count(int count) override { return count; }
    int reset() override {
        SDRGPU_HIP(hipMemset(state.p, 0, sizeof(float2)));
        return SDRGPU_OK;
    }
    template <typename DT>
    void run_t(const void* in, int count, void* out, hipStream_t s) {
        hipLaunchKernelGGL(dcb_kernel<DT>, dim3(1), dim3(LOOP_NT), 0, s, (const DT*)in, (DT*)out, count, rate, state.as<float2>());
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("dc_blocker: negative count"); return SDRGPU_EARG; }
        if (count == 0) return 0;
        if (in_dtype == SDRGPU_C64) run_t<float2>(in, count, out, s);
        else run_t<float>(in, count, out, s);
        SDRGPU_HIP(hipGetLastError());
        return count;
    }
};

struct NoiseBlankerBlock : Block {
    NbParams p{};
    DevBuf state;
    void set(double rate, double level) {   // init / setRate / setLevel (noise_blanker.h:12-30): members are float
        p.rate = (float)rate;
        p.invRate = 1.0f - p.rate;
        p.level = (float)level;
    }
    int setup(int dev, double rate, double level) {
        device = dev;
        in_dtype = out_dtype = SDRGPU_C64;
        set(rate, level);
        SDRGPU_CHECK(state.ensure(sizeof(float)));
        return reset();
    }
    int out_count(int count) override { return count; }
    int reset() override {   // noise_blanker.h:32-36
        const float one = 1.0f;
        SDRGPU_HIP(hipMemcpy(state.p, &one, sizeof(one), hipMemcpyHostToDevice));
        return SDRGPU_OK;
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("noise_blanker: negative count"); return SDRGPU_EARG; }
        if (count == 0) return 0;
        hipLaunchKernelGGL(noise_blanker_kernel, dim3(1), dim3(LOOP_NT), 0, s, (const float2*)in, (float2*)out, count, p,
                           state.as<float>());
        SDRGPU_HIP(hipGetLastError());
        return count;
    }
};

struct DeempBlock : Block {
    float alpha = 1.0f;
    DevBuf state;
    int setup(int dev, int dtype, double tau, double samplerate) {
        device = dev;
        in_dtype = out_dtype = dtype;                 // F32 (float) or C64 (stereo_t)
        set_alpha(tau, samplerate);
        SDRGPU_CHECK(state.ensure(sizeof(float2)));
        return reset();
    }
    void set_alpha(double tau, double samplerate) {   // updateAlpha (deephasis.h:90-93)
        const float dt = (float)(1.0f / samplerate);
        alpha = (float)((double)dt / (tau + (double)dt));
    }
    int out_count(int count) override { return count; }
    int reset() override {
        SDRGPU_HIP(hipMemset(state.p, 0, sizeof(float2)));
        return SDRGPU_OK;
    }
    template <int C>
    void run_t(const void* in, int count, void* out, hipStream_t s) {
        hipLaunchKernelGGL(deemp_kernel<C>, dim3(1), dim3(LOOP_NT), 0, s, (const float*)in, (float*)out, count, alpha, state.as<float2>());
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("deemphasis: negative count"); return SDRGPU_EARG; }
        if (count == 0) return 0;     // (the reference reads out[-1] for count == 0)
        if (in_dtype == SDRGPU_C64) run_t<2>(in, count, out, s);
        else run_t<1>(in, count, out, s);
        SDRGPU_HIP(hipGetLastError());
        return count;
    }
};

// elementwise converters used inside the demod chains
enum class MapKind { Magnitude, RealPart, MonoToStereo };   // c64 -> f32, c64 -> f32, f32 -> c64
struct MapBlock : Block {
    MapKind kind = MapKind::Magnitude;
    int out_count(int count) override { return count; }
    int reset() override { return SDRGPU_OK; }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count <= 0) return count < 0 ? SDRGPU_EARG : 0;
        const dim3 g((count + 255) / 256), b(256);
        switch (kind) {
        case MapKind::Magnitude: hipLaunchKernelGGL(magnitude_kernel, g, b, 0, s, (const float2*)in, (float*)out, count); break;
        case MapKind::RealPart: hipLaunchKernelGGL(real_part_kernel, g, b, 0, s, (const float2*)in, (float*)out, count); break;
        case MapKind::MonoToStereo: hipLaunchKernelGGL(mono_to_stereo_kernel, g, b, 0, s, (const float*)in, (float2*)out, count); break;
        }
        SDRGPU_HIP(hipGetLastError());
        return count;
    }
};

// BroadcastFM (demod/broadcast_fm.h:34-60, 144-215): quadrature -> [stereo: pilot band-pass
// (complex, 305 taps at 240 kS/s) -> PLL -> matrix] -> audio low-pass -> stereo_t
struct BroadcastFmBlock : Block {
    // configuration
    bool stereo = true, lowPass = true;
    bool rds = false;                        // setRDSOut; off unless set_rds(true)
    double fs = 0.0;
    PllParams pp{};
    float initPhase = 0.0f, initFreq = 0.0f;
    int delay = 0;                           // lprDelay / lmrDelay: the pilot filter's group delay
    // sub-blocks. RDS branch (broadcast_fm.h:164-171, 193-203): MPX as complex ->
    // FrequencyXlator(-57 kHz) -> RationalResampler<complex_t>(fs -> 5 kHz), built at the first set_rds(true)
    std::unique_ptr<Block> quad, pilot, audio, rdsChain;
    // state: PLL (phase, freq) and the delay line's last `delay` MPX samples, ping-pong
    DevBuf pllState, hist[2];
    int cur = 0;
    int rdsN = 0;                            // RDS samples of the last call (in rdsOut)
    // scratch of one call
    DevBuf mpx, cplx, pf, ph, lr, rdsIn, rdsOut;

    int set_rds(bool on) {
        rds = on;
        rdsN = 0;
        if (on && !rdsChain) {
            int rc;
            rdsChain.reset(make_xlate_resample_block(device, fs, 5000.0, hz_to_rads(-57000.0, fs), &rc));
            if (rc < 0) { rdsChain.reset(); rds = false; return rc; }
        }
        return SDRGPU_OK;
    }
    int setup(int dev, double deviation, double samplerate, bool st, bool lp) {
        device = dev;
        in_dtype = SDRGPU_C64;
        out_dtype = SDRGPU_C64;
        stereo = st;
        lowPass = lp;
        fs = samplerate;
        int rc;
        quad.reset(make_quad_block(dev, hz_to_rads(deviation, samplerate), &rc));
        SDRGPU_CHECK(rc);
        const int np = taps_band_pass_c(18750.0, 19250.0, 3000.0, samplerate, 1, nullptr);
        if (np < 1) return np < 0 ? np : SDRGPU_EARG;
        std::vector<float> pt(2 * (size_t)np);
        taps_band_pass_c(18750.0, 19250.0, 3000.0, samplerate, 1, pt.data());
        pilot.reset(make_fir_block(dev, SDRGPU_C64, SDRGPU_C64, pt.data(), np, 1, false, &rc));
        SDRGPU_CHECK(rc);
        delay = ((np - 1) / 2) + 1;
        // PLL(25000 / fs, 0, 19 kHz, 18.75 kHz, 19.25 kHz) (broadcast_fm.h:47)
        critically_damped(25000.0 / samplerate, &pp.alpha, &pp.beta);
        pp.minPhase = -3.1415926535f;
        pp.maxPhase = 3.1415926535f;
        pp.phaseDelta = pp.maxPhase - pp.minPhase;
        pp.minFreq = (float)hz_to_rads(18750.0, samplerate);
        pp.maxFreq = (float)hz_to_rads(19250.0, samplerate);
        initPhase = 0.0f;
        initFreq = (float)hz_to_rads(19000.0, samplerate);
        std::vector<float> at;
        SDRGPU_CHECK(design_taps(at, taps_low_pass, 15000.0, 4000.0, samplerate, 0));
        if (!lowPass) { at.assign(1, 1.0f); }                          // identity: raw L/R (or MPX) pairs
        // (l, r) pairs filtered as one complex stream with real taps = alFir / arFir
        audio.reset(make_fir_block(dev, SDRGPU_C64, SDRGPU_F32, at.data(), (int)at.size(), 1, false, &rc));
        SDRGPU_CHECK(rc);
        SDRGPU_CHECK(pllState.ensure(sizeof(float2)));
        for (int k = 0; k < 2; k++) SDRGPU_CHECK(hist[k].ensure(sizeof(float) * delay));
        return reset();
    }
    int out_count(int count) override { return count; }
    int reset() override {   // broadcast_fm.h:130-142: not the RDS branch, whose NCO phase and resampler history survive
        SDRGPU_CHECK(quad->reset());
        SDRGPU_CHECK(pilot->reset());
        SDRGPU_CHECK(audio->reset());
        const float2 st = make_float2(initPhase, initFreq);
        SDRGPU_HIP(hipMemcpy(pllState.p, &st, sizeof(st), hipMemcpyHostToDevice));
        SDRGPU_HIP(hipMemset(hist[cur].p, 0, sizeof(float) * delay));
        return SDRGPU_OK;
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("broadcast_fm: negative count"); return SDRGPU_EARG; }
        rdsN = 0;
        if (count == 0) return 0;
        SDRGPU_CHECK(mpx.ensure(sizeof(float) * count));
        SDRGPU_CHECK(lr.ensure(sizeof(float2) * count));
        int m = quad->run(in, count, mpx.p, s);
        if (m < 0) return m;
        const dim3 g((count + 255) / 256), b(256);
        if (stereo) {
            SDRGPU_CHECK(cplx.ensure(sizeof(float2) * count));
            SDRGPU_CHECK(pf.ensure(sizeof(float2) * count));
            SDRGPU_CHECK(ph.ensure(sizeof(float) * count));
            hipLaunchKernelGGL(real_to_complex_kernel, g, b, 0, s, mpx.as<float>(), cplx.as<float2>(), count);
            m = pilot->run(cplx.p, count, pf.p, s);
            if (m < 0) return m;
            hipLaunchKernelGGL(phase_kernel, g, b, 0, s, pf.as<float2>(), ph.as<float>(), count);
            hipLaunchKernelGGL(pll_kernel, dim3(1), dim3(LOOP_NT), 0, s, ph.as<float>(), count, pp, pllState.as<float2>());
            hipLaunchKernelGGL(stereo_matrix_kernel, g, b, 0, s, mpx.as<float>(), hist[cur].as<float>(), delay,
                               ph.as<float>(), lr.as<float2>(), count);
            SDRGPU_CHECK(carry_history(SDRGPU_F32, nullptr, hist[cur], mpx.p, hist[cur ^ 1], delay, count, s));
            cur ^= 1;
        } else {
            hipLaunchKernelGGL(mono_to_stereo_kernel, g, b, 0, s, mpx.as<float>(), lr.as<float2>(), count);
        }
        SDRGPU_HIP(hipGetLastError());
        if (rds && rdsChain) {
            // the undelayed MPX as complex (the stereo path already holds it in cplx)
            const float2* c = cplx.as<float2>();
            if (!stereo) {
                SDRGPU_CHECK(rdsIn.ensure(sizeof(float2) * count));
                hipLaunchKernelGGL(real_to_complex_kernel, g, b, 0, s, mpx.as<float>(), rdsIn.as<float2>(), count);
                SDRGPU_HIP(hipGetLastError());
                c = rdsIn.as<float2>();
            }
            const int want = rdsChain->out_count(count);
            if (want < 0) return want;
            SDRGPU_CHECK(rdsOut.ensure(sizeof(float2) * (size_t)std::max(want, 1)));
            rdsN = rdsChain->run(c, count, rdsOut.p, s);
            if (rdsN < 0) return rdsN;
        }
        return audio->run(lr.p, count, out, s);
    }
};

// ---------------------------------------------------------- chain building
static int append_map(Block* chain, int dev, MapKind kind) {
    auto* m = new MapBlock();
    m->device = dev;
    m->kind = kind;
    m->in_dtype = kind == MapKind::MonoToStereo ? SDRGPU_F32 : SDRGPU_C64;
    m->out_dtype = kind == MapKind::MonoToStereo ? SDRGPU_C64 : SDRGPU_F32;
    return chain_append(chain, m);
}
// the AGC of AM (am.h:27-49) and SSB (ssb.h:27-40): set point 1, max gain 10e6, max output 10, initial
// gain inf; of CW (cw.h:20): max output 1, initial gain 1; `enabled` false = the fixed-gain limiter
// (setAGCGain path)
static AgcBlock* make_demod_agc(int dev, int dtype, double attack, double decay, bool enabled, int* rc,
                                double maxOutputAmp = 10.0, double initGain = INFINITY) {
    auto* a = new AgcBlock();
    *rc = a->setup(dev, dtype, 1.0, attack, decay, 10e6, maxOutputAmp, initGain);
    a->p.enabled = enabled ? 1 : 0;
    return a;
}
// xlate -> Re -> AGC [-> MonoToStereo] (ssb.h:90-105, cw.h:72-85) into the new chain *c; *xl: its xlator
static int xlate_agc_chain(int device, double offsetRad, bool agcEnabled, double attack, double decay, double maxOutputAmp,
                           double initGain, bool stereo, Block** c, Block** xl = nullptr) {
    *c = chain_new(device, SDRGPU_C64, stereo ? SDRGPU_C64 : SDRGPU_F32);
    int rc;
    Block* x = make_xlator_block(device, offsetRad, &rc);
    if (xl) *xl = x;
    rc = append_owned(*c, x, rc);
    if (rc >= 0) rc = append_map(*c, device, MapKind::RealPart);
    if (rc >= 0) {
        Block* a = make_demod_agc(device, SDRGPU_F32, attack, decay, agcEnabled, &rc, maxOutputAmp, initGain);
        rc = append_owned(*c, a, rc);
    }
    if (rc >= 0 && stereo) rc = append_map(*c, device, MapKind::MonoToStereo);
    return rc;
}
// demod::CW<T> (cw.h): the chain above behind a block of its own, which knows the sample rate of setTone
struct CwBlock : Block {
    std::unique_ptr<Block> chain;
    Block* xlator = nullptr;   // (the chain's)
    double samplerate = 1.0;
    int out_count(int count) override { return chain->out_count(count); }
    int reset() override { return chain->reset(); }
    int run(const void* in, int count, void* out, hipStream_t s) override { return chain->run(in, count, out, s); }
};
// AGC access inside the AM / SSB / CW chains: `which` 0 = the first AGC of the chain (AM carrier
// AGC in CARRIER mode, the SSB and CW AGC), 1 = the last (AM audio AGC)
static AgcBlock* demod_agc(sdrgpu_block* h, int which) {
    Block* chain = h ? h->impl : nullptr;
    if (auto* cw = dynamic_cast<CwBlock*>(chain)) chain = cw->chain.get();
    AgcBlock* a = find_kid<AgcBlock>(chain, which != 0);
    if (!a) set_error("demod has no AGC");
    return a;
}
}  // namespace sdrgpu

using namespace sdrgpu;

// ------------------------------------------------------------------- C ABI
extern "C" int sdrgpu_agc_create(sdrgpu_block** h, int device, int dtype, double setPoint, double attack, double decay,
                                 double maxGain, double maxOutputAmp, double initGain) {
    if (!h || (dtype != SDRGPU_F32 && dtype != SDRGPU_C64)) { set_error("agc_create: bad argument"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    auto* a = new AgcBlock();
    return publish_block(h, a, a->setup(device, dtype, setPoint, attack, decay, maxGain, maxOutputAmp, initGain));
}
// AGC setters (agc.h:44-79): parameters change, the running amplitude / gain are kept
extern "C" int sdrgpu_agc_set_params(sdrgpu_block* h, double setPoint, double attack, double decay, double maxGain,
                                     double maxOutputAmp, double initGain) {
    auto* a = h ? dynamic_cast<AgcBlock*>(h->impl) : nullptr;
    if (!a) { set_error("not an AGC"); return SDRGPU_EARG; }
    a->set_params(setPoint, attack, decay, maxGain, maxOutputAmp, initGain);
    return SDRGPU_OK;
}
extern "C" int sdrgpu_agc_set_enabled(sdrgpu_block* h, int enabled) {
    auto* a = h ? dynamic_cast<AgcBlock*>(h->impl) : nullptr;
    if (!a) { set_error("not an AGC"); return SDRGPU_EARG; }
    a->p.enabled = enabled ? 1 : 0;
    return SDRGPU_OK;
}
extern "C" int sdrgpu_agc_set_gain(sdrgpu_block* h, float gain) {
    auto* a = h ? dynamic_cast<AgcBlock*>(h->impl) : nullptr;
    if (!a) { set_error("not an AGC"); return SDRGPU_EARG; }
    SDRGPU_CHECK(enter_block(h, true));   // (a queued call may still read the latched gain's device word)
    return a->set_gain(gain);
}
extern "C" int sdrgpu_agc_get_gain(sdrgpu_block* h, float* gain) {
    auto* a = h ? dynamic_cast<AgcBlock*>(h->impl) : nullptr;
    if (!a || !gain) { set_error("agc_get_gain: bad argument"); return SDRGPU_EARG; }
    SDRGPU_CHECK(enter_block(h, !a->pending));   // (UI-rate query: waits for the block's queued work)
    return a->get_gain(gain);
}

extern "C" int sdrgpu_dc_blocker_create(sdrgpu_block** h, int device, int dtype, double rate) {
    if (!h || (dtype != SDRGPU_F32 && dtype != SDRGPU_C64)) { set_error("dc_blocker_create: bad argument"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    auto* d = new DcbBlock();
    return publish_block(h, d, d->setup(device, dtype, rate));
}
extern "C" int sdrgpu_dc_blocker_set_rate(sdrgpu_block* h, double rate) {
    DcbBlock* d = h ? dynamic_cast<DcbBlock*>(h->impl) : nullptr;
    if (!d) d = find_kid<DcbBlock>(h, false);   // the AM chain's DC blocker
    if (!d) { set_error("no DC blocker"); return SDRGPU_ESTATE; }
    d->rate = (float)rate;
    return SDRGPU_OK;
}

// noise_reduction::NoiseBlanker (noise_blanker.h): the setters keep the running amplitude
extern "C" int sdrgpu_noise_blanker_create(sdrgpu_block** h, int device, double rate, double level) {
    if (!h) { set_error("noise_blanker_create: null handle pointer"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    auto* b = new NoiseBlankerBlock();
    return publish_block(h, b, b->setup(device, rate, level));
}
extern "C" int sdrgpu_noise_blanker_set(sdrgpu_block* h, double rate, double level) {
    auto* b = h ? dynamic_cast<NoiseBlankerBlock*>(h->impl) : nullptr;
    if (!b) { set_error("not a noise blanker"); return SDRGPU_EARG; }
    b->set(rate, level);
    return SDRGPU_OK;
}

// filter::Deemphasis<T> (deephasis.h): dtype F32 (float) or C64 (stereo_t)
extern "C" int sdrgpu_deemphasis_create(sdrgpu_block** h, int device, int dtype, double tau, double samplerate) {
    if (!h || (dtype != SDRGPU_F32 && dtype != SDRGPU_C64) || !(samplerate > 0)) { set_error("deemphasis_create: bad argument"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    auto* d = new DeempBlock();
    return publish_block(h, d, d->setup(device, dtype, tau, samplerate));
}
extern "C" int sdrgpu_deemphasis_set(sdrgpu_block* h, double tau, double samplerate) {   // setTau / setSamplerate
    auto* d = h ? dynamic_cast<DeempBlock*>(h->impl) : nullptr;
    if (!d || !(samplerate > 0)) { set_error("not a deemphasis block"); return SDRGPU_EARG; }
    d->set_alpha(tau, samplerate);
    return SDRGPU_OK;
}

// demod::AM<T> (am.h:27-49, 114-142): agcMode 0 OFF, 1 CARRIER, 2 AUDIO; stereo -> stereo_t out
extern "C" int sdrgpu_am_create(sdrgpu_block** h, int device, int agcMode, double bandwidth, double agcAttack,
                                double agcDecay, double dcBlockRate, double samplerate, int stereo) {
    if (!h || agcMode < 0 || agcMode > 2) { set_error("am_create: bad argument"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    Block* c = chain_new(device, SDRGPU_C64, stereo ? SDRGPU_C64 : SDRGPU_F32);
    int rc = SDRGPU_OK;
    if (agcMode == 1) {
        Block* a = make_demod_agc(device, SDRGPU_C64, agcAttack, agcDecay, true, &rc);
        rc = append_owned(c, a, rc);
    }
    if (rc >= 0) rc = append_map(c, device, MapKind::Magnitude);
    if (rc >= 0) {
        auto* d = new DcbBlock();
        rc = append_owned(c, d, d->setup(device, SDRGPU_F32, dcBlockRate));
    }
    if (rc >= 0 && agcMode != 1) {   // audioAgc runs unless CARRIER; enabled only for AUDIO
        Block* a = make_demod_agc(device, SDRGPU_F32, agcAttack, agcDecay, agcMode == 2, &rc);
        rc = append_owned(c, a, rc);
    }
    if (rc >= 0) {
        const double fc = bandwidth / 2.0;
        std::vector<float> t;
        rc = design_taps(t, taps_low_pass, fc, fc * 0.1, samplerate, 0);
        if (rc >= 0) {
            Block* f = make_fir_block(device, SDRGPU_F32, SDRGPU_F32, t.data(), (int)t.size(), 1, stereo != 0, &rc);
            rc = append_owned(c, f, rc);
            if (rc >= 0) rc = chain_keep_on_reset(c, 1);   // reset() (am.h:104-112): the AGCs and the DC blocker, not lpf
        }
    }
    return publish_block(h, c, rc);
}

// demod::SSB<T> (ssb.h:27-105): mode 0 USB, 1 LSB, 2 DSB
extern "C" int sdrgpu_ssb_create(sdrgpu_block** h, int device, int mode, double bandwidth, double samplerate,
                                 int agcEnabled, double agcAttack, double agcDecay, int stereo) {
    if (!h || mode < 0 || mode > 2) { set_error("ssb_create: bad argument"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    Block* c = nullptr;
    const double tr = mode == 0 ? bandwidth / 2.0 : (mode == 1 ? -bandwidth / 2.0 : 0.0);   // getTranslation
    const int rc = xlate_agc_chain(device, hz_to_rads(tr, samplerate), agcEnabled != 0, agcAttack, agcDecay, 10.0, INFINITY, stereo != 0, &c);
    return publish_block(h, c, rc);
}

// demod::CW<T> (cw.h:15-28, 72-85): the SSB chain with the tone as translation and the AGC's max output and
// initial gain at 1 (cw.h:20)
extern "C" int sdrgpu_cw_create(sdrgpu_block** h, int device, double tone, int agcEnabled, double agcAttack, double agcDecay,
                                double samplerate, int stereo) {
    if (!h || !std::isfinite(tone) || !std::isfinite(samplerate) || !(samplerate > 0)) { set_error("cw_create: bad argument"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    auto* w = new CwBlock();
    w->device = device;
    w->in_dtype = SDRGPU_C64;
    w->out_dtype = stereo ? SDRGPU_C64 : SDRGPU_F32;
    w->samplerate = samplerate;
    Block* c = nullptr;
    const int rc = xlate_agc_chain(device, hz_to_rads(tone, samplerate), agcEnabled != 0, agcAttack, agcDecay, 1.0, 1.0, stereo != 0, &c, &w->xlator);
    w->chain.reset(c);
    return publish_block(h, w, rc);
}
// CW::setTone (cw.h:30-35): the xlator's offset changes, its phase is kept
extern "C" int sdrgpu_cw_set_tone(sdrgpu_block* h, double tone) {
    if (!h || !h->impl) { set_error("null block handle"); return SDRGPU_EARG; }
    auto* w = dynamic_cast<CwBlock*>(h->impl);
    if (!w) { set_error("not a CW block"); return SDRGPU_ESTATE; }
    if (!std::isfinite(tone)) { set_error("cw_set_tone: tone not finite"); return SDRGPU_EARG; }
    SDRGPU_CHECK(enter_block(h, true));   // (a queued call still reads the fine table that the setter rewrites)
    return xlator_block_set_offset(w->xlator, hz_to_rads(tone, w->samplerate));
}

extern "C" int sdrgpu_demod_agc_set_gain(sdrgpu_block* h, int which, float gain) {
    AgcBlock* a = demod_agc(h, which);
    if (!a) return SDRGPU_ESTATE;
    SDRGPU_CHECK(enter_block(h, true));
    return a->set_gain(gain);
}
extern "C" int sdrgpu_demod_agc_get_gain(sdrgpu_block* h, int which, float* gain) {
    AgcBlock* a = demod_agc(h, which);
    if (!a) return SDRGPU_ESTATE;
    if (!gain) { set_error("agc_get_gain: bad argument"); return SDRGPU_EARG; }
    SDRGPU_CHECK(enter_block(h, !a->pending));
    return a->get_gain(gain);
}
extern "C" int sdrgpu_demod_agc_set_enabled(sdrgpu_block* h, int which, int enabled) {
    AgcBlock* a = demod_agc(h, which);
    if (!a) return SDRGPU_ESTATE;
    a->p.enabled = enabled ? 1 : 0;
    return SDRGPU_OK;
}
// (an AM or SSB chain holds one AGC: the carrier AGC in CARRIER mode, else the audio AGC)
extern "C" int sdrgpu_demod_agc_set_attack_decay(sdrgpu_block* h, double attack, double decay) {
    if (!h || !h->impl) { set_error("null block handle"); return SDRGPU_EARG; }
    AgcBlock* a = demod_agc(h, 0);
    if (!a) return SDRGPU_ESTATE;
    a->set_attack_decay(attack, decay);
    return SDRGPU_OK;
}

// demod::BroadcastFM (broadcast_fm.h), stereo decoder and RDS branch included
extern "C" int sdrgpu_broadcast_fm_create(sdrgpu_block** h, int device, double deviation, double samplerate, int stereo,
                                          int lowPass) {
    if (!h || !(samplerate > 0)) { set_error("broadcast_fm_create: bad argument"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    auto* w = new BroadcastFmBlock();
    return publish_block(h, w, w->setup(device, deviation, samplerate, stereo != 0, lowPass != 0));
}
extern "C" int sdrgpu_broadcast_fm_set_rds(sdrgpu_block* h, int enabled) {   // setRDSOut (broadcast_fm.h:121-127)
    auto* w = h ? dynamic_cast<BroadcastFmBlock*>(h->impl) : nullptr;
    if (!w) { set_error("not a broadcast_fm block"); return SDRGPU_EARG; }
    SDRGPU_CHECK(enter_block(h));
    const bool built = enabled && !w->rdsChain;
    SDRGPU_CHECK(w->set_rds(enabled != 0));
    if (built) SDRGPU_HIP(hipDeviceSynchronize());   // the new RDS chain's histories, zeroed on the null stream (blocks.h)
    return SDRGPU_OK;
}
// RDS samples (complex_t at 5 kS/s) of the last process call: device pointer and count
extern "C" int sdrgpu_broadcast_fm_rds_dev(sdrgpu_block* h, const void** out, int* n) {
    auto* w = h ? dynamic_cast<BroadcastFmBlock*>(h->impl) : nullptr;
    if (!w) { set_error("not a broadcast_fm block"); return SDRGPU_EARG; }
    if (out) *out = w->rdsOut.p;
    if (n) *n = w->rds ? w->rdsN : 0;
    return w->rds ? w->rdsN : 0;
}
extern "C" int sdrgpu_broadcast_fm_read_rds(sdrgpu_block* h, void* out, int max) {   // host copy (waits for the block)
    auto* w = h ? dynamic_cast<BroadcastFmBlock*>(h->impl) : nullptr;
    if (!w || (!out && max > 0)) { set_error("broadcast_fm_read_rds: bad argument"); return SDRGPU_EARG; }
    const int n = std::min(max, w->rds ? w->rdsN : 0);
    if (n <= 0) return 0;
    SDRGPU_CHECK(enter_block(h, true));
    SDRGPU_HIP(hipMemcpy(out, w->rdsOut.p, sizeof(float2) * (size_t)n, hipMemcpyDeviceToHost));
    return n;
}
