// Host side of symbol recovery (the kernels are in symsync_kernels.h, which also says why this file is
// built with -ffp-contract=off):
//   loop::FastAGC<T>, loop::Costas<ORDER>, clock_recovery::MM<T>, digital::BinarySlicer,
//   digital::DifferentialDecoder
//   demod::PSK<ORDER>   demod/psk.h:25-43, 138-143   (RRC FIR -> FastAGC -> Costas -> MM<complex_t>)
//   demod::GFSK         demod/gfsk.h:24-41, 131-135  (Quadrature -> RRC FIR -> MM<float>)
//   the RDS chain       decoder_modules/radio/src/demodulators/wfm.h:57-68
//   loop::PLL, loop::CarrierTrackingPLL   loop/pll.h:15-70, loop/carrier_tracking_pll.h:14-20
//   loop::MeteorCostas, demod::Meteor     decoder_modules/meteor_demodulator/src/meteor_costas.h:13-56,
//                       meteor_demod.h:24-43, 139-167 (RRC FIR in the reference's order -> FastAGC -> MeteorCostas with
//                       the OQPSK stagger -> MM<complex_t>)
// Top to bottom: the block structs (each: configuration, state, setup / reset, its launch in run), the
// C entry points. The structs select no device and own no stream: an entry point does, through
// enter_block or, for a create, itself and publish_block (blocks.h, which also states when an entry
// point waits for the device).
#include <algorithm>
#include <cmath>
#include <vector>
#include "sdrgpu_internal.h"
#include "blocks.h"
#include "symsync_kernels.h"
#include "symsync_args.h"   // the argument checks, shared with bank.hip

namespace sdrgpu {

struct FastAgcBlock : Block {
    FastAgcParams p{};
    float initGain = 1.0f;
    DevBuf state;
    void set(double setPoint, double maxGain, double rate, double initGain_) {
        fast_agc_params(p, setPoint, maxGain, rate);
        initGain = (float)initGain_;
    }
    int setup(int dev, int dtype, double setPoint, double maxGain, double rate, double initGain_) {
        device = dev;
        in_dtype = out_dtype = dtype;
        set(setPoint, maxGain, rate, initGain_);
        SDRGPU_CHECK(state.ensure(sizeof(float)));
        return reset();
    }
    int out_count(int count) override { return count; }
    int reset() override {   // fast_agc.h:54-58
        SDRGPU_HIP(hipMemcpy(state.p, &initGain, sizeof(float), hipMemcpyHostToDevice));
        p.hasGain = 0;
        return SDRGPU_OK;
    }
    void set_gain(double g) {   // fast_agc.h:48-52, applied at the next call
        p.setGain = (float)g;
        p.hasGain = 1;
    }
    int get_gain(float* gain) {   // (the caller has waited for the block's queued work unless a gain is latched)
        if (p.hasGain) { *gain = p.setGain; return SDRGPU_OK; }
        SDRGPU_HIP(hipMemcpy(gain, state.p, sizeof(float), hipMemcpyDeviceToHost));
        return SDRGPU_OK;
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("fast_agc: negative count"); return SDRGPU_EARG; }
        if (count == 0) return 0;   // (a latched gain waits for the next samples)
        if (in_dtype == SDRGPU_C64)
            hipLaunchKernelGGL(fast_agc_kernel<float2>, dim3(1), dim3(LOOP_NT), 0, s, (const float2*)in, (float2*)out, count, p, state.as<float>());
        else
            hipLaunchKernelGGL(fast_agc_kernel<float>, dim3(1), dim3(LOOP_NT), 0, s, (const float*)in, (float*)out, count, p, state.as<float>());
        p.hasGain = 0;
        SDRGPU_HIP(hipGetLastError());
        return count;
    }
};

struct CostasBlock : Block {
    int order = 2;
    CostasParams p{};
    float initPhase = 0.0f, initFreq = 0.0f;
    DevBuf state;
    int setup(int dev, int order_, double bandwidth, double initPhase_, double initFreq_, double minFreq, double maxFreq) {
        device = dev;
        in_dtype = out_dtype = SDRGPU_C64;
        order = order_;
        critically_damped(bandwidth, &p.pcl.alpha, &p.pcl.beta);
        p.pcl.minFreq = (float)minFreq;
        p.pcl.maxFreq = (float)maxFreq;
        initPhase = (float)initPhase_;
        initFreq = (float)initFreq_;
        SDRGPU_CHECK(state.ensure(sizeof(float2)));
        return reset();
    }
    int out_count(int count) override { return count; }
    int reset() override {   // pll.h:55-62
        const float2 st = make_float2(initPhase, initFreq);
        SDRGPU_HIP(hipMemcpy(state.p, &st, sizeof(st), hipMemcpyHostToDevice));
        return SDRGPU_OK;
    }
    template <int ORDER>
    void run_t(const void* in, int count, void* out, hipStream_t s) {
        hipLaunchKernelGGL(costas_kernel<ORDER>, dim3(1), dim3(LOOP_NT), 0, s, (const float2*)in, (float2*)out, count, p, state.as<float2>());
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("costas: negative count"); return SDRGPU_EARG; }
        if (count == 0) return 0;
        if (order == 2) run_t<2>(in, count, out, s);
        else if (order == 4) run_t<4>(in, count, out, s);
        else run_t<8>(in, count, out, s);
        p.clampNow = 0;
        SDRGPU_HIP(hipGetLastError());
        return count;
    }
};

// filter::FIR<complex_t, float> (filter/fir.h:60-80) summed as the reference's VOLK generic kernel sums it: ascending
// taps, fp32, unfused -- the stream banks' FIR kernel on one stream, the host side of BankFir (bank.hip). demod::Meteor's
// RRC: with it the chain differs from the reference by the loop's libm alone, and a BankMeteor column is this chain
// bit for bit. (FirBlock, blocks.hip, picks its kernel and summation order by shape and contracts: it is held to a
// tolerance, and PSK / GFSK keep it.)
struct OrderedFirBlock : Block {
    std::vector<float> taps;
    DevBuf tapsDev, hist[2];   // hist[cur]: the T - 1 samples before the next call's first
    int cur = 0;
    int H() const { return (int)taps.size() - 1; }
    int setup(int dev, const float* t, int n) {
        device = dev;
        in_dtype = out_dtype = SDRGPU_C64;
        taps.assign(t, t + n);
        SDRGPU_CHECK(tapsDev.ensure(sizeof(float) * taps.size()));
        SDRGPU_HIP(hipMemcpy(tapsDev.p, taps.data(), sizeof(float) * taps.size(), hipMemcpyHostToDevice));
        for (auto& b : hist) SDRGPU_CHECK(b.ensure(sizeof(float2) * (size_t)std::max(H(), 1)));
        return reset();
    }
    int out_count(int count) override { return count; }
    int reset() override {   // fir.h:49-53
        SDRGPU_HIP(hipMemset(hist[cur].p, 0, hist[cur].bytes));
        return SDRGPU_OK;
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("fir: negative count"); return SDRGPU_EARG; }
        if (count == 0) return 0;
        hipLaunchKernelGGL(bank_fir_kernel<float2>, dim3((count + 255) / 256), dim3(256), 0, s, (const float2*)in, (float2*)out, count,
                           1, H(), tapsDev.as<float>(), (int)taps.size(), hist[cur].as<float2>());
        SDRGPU_HIP(hipGetLastError());
        if (H() > 0) {
            SDRGPU_CHECK(carry_history(SDRGPU_C64, nullptr, hist[cur], in, hist[cur ^ 1], H(), count, s));
            cur ^= 1;
        }
        return count;
    }
};

// loop::MeteorCostas (meteor_costas.h:6-59) is a PLL with its own process, as Costas<ORDER> is: the block is a
// CostasBlock (coefficients, limits, initial state, reset; the Costas setters reach it) with its own launch.
struct MeteorCostasBlock : CostasBlock {
    int broken = 0, oqpsk = 0;
    DevBuf lastI;   // demod::Meteor's stagger carry (meteor_demod.h:188): 0 at create, no reset touches it
    int setup(int dev, double bandwidth, int broken_, int oqpsk_, double initPhase_, double initFreq_, double minFreq, double maxFreq) {
        broken = broken_ ? 1 : 0;
        oqpsk = oqpsk_ ? 1 : 0;
        SDRGPU_CHECK(lastI.ensure(sizeof(float)));
        SDRGPU_HIP(hipMemset(lastI.p, 0, sizeof(float)));
        return CostasBlock::setup(dev, 4, bandwidth, initPhase_, initFreq_, minFreq, maxFreq);
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("meteor_costas: negative count"); return SDRGPU_EARG; }
        if (count == 0) return 0;
        const MeteorCostasParams mp{p, broken, oqpsk};
        hipLaunchKernelGGL(meteor_costas_kernel, dim3(1), dim3(LOOP_NT), 0, s, (const float2*)in, (float2*)out, count, mp,
                           state.as<float2>(), lastI.as<float>());
        p.clampNow = 0;
        SDRGPU_HIP(hipGetLastError());
        return count;
    }
};

// loop::PLL (pll.h:8-89) and loop::CarrierTrackingPLL (carrier_tracking_pll.h:5-21): a CostasBlock likewise, run by
// the phase-control-loop step BroadcastFM's pilot PLL runs (pll_step, loop_steps.h)
struct PllBlock : CostasBlock {
    bool derotate = false;
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("pll: negative count"); return SDRGPU_EARG; }
        if (count == 0) return 0;
        const PllParams pp = pll_params(p.pcl);
        if (derotate)
            hipLaunchKernelGGL(carrier_pll_kernel<true>, dim3(1), dim3(LOOP_NT), 0, s, (const float2*)in, (float2*)out, count, pp,
                               p.clampNow, state.as<float2>());
        else
            hipLaunchKernelGGL(carrier_pll_kernel<false>, dim3(1), dim3(LOOP_NT), 0, s, (const float2*)in, (float2*)out, count, pp,
                               p.clampNow, state.as<float2>());
        p.clampNow = 0;
        SDRGPU_HIP(hipGetLastError());
        return count;
    }
};

struct MmBlock : Block {
    MmParams p{};
    MmEpilogue epi = MmEpilogue::Soft;
    double omega = 0.0, omegaGain = 0.0, muGain = 0.0, rel = 0.0;
    DevBuf state, hist, bank, soft;
    PinnedBuf countBuf;   // the call's output count, read back at the end of run()
    int lastCount = 0;
    void set_pcl() { mm_pcl_params(p, omega, omegaGain, muGain, rel); }
    int setup(int dev, int dtype, MmEpilogue e, int inStride, double omega_, double omegaGain_, double muGain_, double rel_,
              int P, int T) {
        device = dev;
        in_dtype = (dtype == SDRGPU_F32 && inStride == 2) ? SDRGPU_C64 : dtype;
        out_dtype = e == MmEpilogue::Soft ? dtype : SDRGPU_U8;
        epi = e;
        omega = omega_; omegaGain = omegaGain_; muGain = muGain_; rel = rel_;
        set_pcl();
        p.P = P;
        p.T = T;
        p.inStride = inStride;
        p.modulus = 2;
        std::vector<float> b((size_t)P * T);
        SDRGPU_CHECK(mm_interp_bank(P, T, b.data()));
        SDRGPU_CHECK(state.ensure(sizeof(MmState)));
        SDRGPU_CHECK(hist.ensure(esize(dtype) * std::max(T - 1, 1)));
        SDRGPU_CHECK(bank.ensure(sizeof(float) * b.size()));
        SDRGPU_CHECK(countBuf.ensure(sizeof(int)));
        SDRGPU_HIP(hipMemcpy(bank.p, b.data(), sizeof(float) * b.size(), hipMemcpyHostToDevice));
        SDRGPU_HIP(hipMemset(hist.p, 0, hist.bytes));   // (the reference's work buffer starts uninitialised)
        return reset();
    }
    // the capacity of a call: at most one output per input sample (mm_params_ok)
    int out_count(int count) override { return count; }
    int reset() override {   // mm.h:87-98: the state, not the history
        MmState s{};
        s.freq = (float)omega;
        SDRGPU_HIP(hipMemcpy(state.p, &s, sizeof(s), hipMemcpyHostToDevice));
        p.setOmega = p.clampNow = 0;
        lastCount = 0;
        return SDRGPU_OK;
    }
    template <typename DT, MmEpilogue E>
    void run_t(const void* in, int count, void* out, hipStream_t s) {
        hipLaunchKernelGGL((mm_kernel<DT, E>), dim3(1), dim3(LOOP_NT), 0, s, (const DT*)in, count, out, soft.as<float>(), p,
                           bank.as<float>(), hist.as<DT>(), state.as<MmState>());
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("mm: negative count"); return SDRGPU_EARG; }
        lastCount = 0;
        if (count == 0) return 0;   // (latched setters wait for the next samples)
        if (epi == MmEpilogue::DiffBits) {
            SDRGPU_CHECK(soft.ensure(sizeof(float) * (size_t)count));
            run_t<float, MmEpilogue::DiffBits>(in, count, out, s);
        } else if (out_dtype == SDRGPU_C64) {
            run_t<float2, MmEpilogue::Soft>(in, count, out, s);
        } else {
            run_t<float, MmEpilogue::Soft>(in, count, out, s);
        }
        p.setOmega = p.clampNow = 0;
        SDRGPU_HIP(hipGetLastError());
        // the data-dependent count: the one wait of the call
        SDRGPU_HIP(hipMemcpyAsync(countBuf.p, &state.as<MmState>()->outCount, sizeof(int), hipMemcpyDeviceToHost, s));
        SDRGPU_HIP(hipStreamSynchronize(s));
        lastCount = *reinterpret_cast<const int*>(countBuf.p);
        return lastCount;
    }
};

struct SlicerBlock : Block {
    int out_count(int count) override { return count; }
    int reset() override { return SDRGPU_OK; }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count <= 0) return count < 0 ? SDRGPU_EARG : 0;
        hipLaunchKernelGGL(slicer_kernel, dim3((count + 255) / 256), dim3(256), 0, s, (const float*)in, (uint8_t*)out, count);
        SDRGPU_HIP(hipGetLastError());
        return count;
    }
};

struct DiffDecoderBlock : Block {
    int modulus = 2, initSym = 0;
    DevBuf last;   // two ints: [cur] the symbol before the next call's first, [cur ^ 1] written by that call
    int cur = 0;
    int setup(int dev, int modulus_, int initSym_) {
        device = dev;
        in_dtype = out_dtype = SDRGPU_U8;
        modulus = modulus_;
        initSym = initSym_;
        SDRGPU_CHECK(last.ensure(2 * sizeof(int)));
        return reset();
    }
    int out_count(int count) override { return count; }
    int reset() override {   // differential_decoder.h:33-39
        SDRGPU_HIP(hipMemcpy(last.as<int>() + cur, &initSym, sizeof(int), hipMemcpyHostToDevice));
        return SDRGPU_OK;
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count <= 0) return count < 0 ? SDRGPU_EARG : 0;
        hipLaunchKernelGGL(diff_decode_kernel, dim3((count + 255) / 256), dim3(256), 0, s, (const uint8_t*)in, (uint8_t*)out, count,
                           modulus, last.as<int>() + cur, last.as<int>() + (cur ^ 1));
        cur ^= 1;
        SDRGPU_HIP(hipGetLastError());
        return count;
    }
};

// ---------------------------------------------------------- chain building
static Block* make_fast_agc(int dev, int dtype, double setPoint, double maxGain, double rate, double initGain, int* rc) {
    auto* a = new FastAgcBlock();
    *rc = a->setup(dev, dtype, setPoint, maxGain, rate, initGain);
    return a;
}
static Block* make_costas(int dev, int order, double bandwidth, double initPhase, double initFreq, double minFreq,
                          double maxFreq, int* rc) {
    auto* c = new CostasBlock();
    *rc = costas_args_ok(order, bandwidth, initPhase, initFreq, minFreq, maxFreq)
              ? c->setup(dev, order, bandwidth, initPhase, initFreq, minFreq, maxFreq) : SDRGPU_EARG;
    return c;
}
static Block* make_mm(int dev, int dtype, MmEpilogue e, int inStride, double omega, double omegaGain, double muGain, double rel,
                      int P, int T, int* rc) {
    auto* m = new MmBlock();
    *rc = mm_args_ok(omega, omegaGain, muGain, rel, P, T) ? m->setup(dev, dtype, e, inStride, omega, omegaGain, muGain, rel, P, T)
                                                          : SDRGPU_EARG;
    return m;
}
// FIR<T, float>(rootRaisedCosine<float>(count, beta, symbolrate, samplerate)) (psk.h:31-32, gfsk.h:32-33)
static Block* make_rrc_fir(int dev, int dtype, int count, double beta, double symbolrate, double samplerate, int* rc) {
    std::vector<float> t;
    *rc = design_taps(t, taps_root_raised_cosine, count, beta, samplerate / symbolrate);
    if (*rc < 0) return nullptr;
    return make_fir_block(dev, dtype, SDRGPU_F32, t.data(), (int)t.size(), 1, false, rc);
}
// the handle's own block, or the first block of that type in its chain (a PSK handle's AGC and Costas loop)
template <typename T>
static T* as_block(sdrgpu_block* h, const char* what) {
    T* b = (h && h->impl) ? dynamic_cast<T*>(h->impl) : nullptr;
    if (!b) b = find_kid<T>(h, false);
    if (!b) set_error("not %s (or a chain holding one)", what);
    return b;
}
// the handle's own MM block, or the one that ends its PSK / GFSK / RDS chain
static MmBlock* mm_of(sdrgpu_block* h) { return as_block<MmBlock>(h, "an MM block"); }
}  // namespace sdrgpu

using namespace sdrgpu;

// ------------------------------------------------------------------- C ABI
extern "C" int sdrgpu_fast_agc_create(sdrgpu_block** h, int device, int dtype, double setPoint, double maxGain, double rate,
                                      double initGain) {
    if (!h || !real_or_complex(dtype)) { set_error("fast_agc_create: bad argument"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    int rc;
    Block* a = make_fast_agc(device, dtype, setPoint, maxGain, rate, initGain, &rc);
    return publish_block(h, a, rc);
}
extern "C" int sdrgpu_fast_agc_set(sdrgpu_block* h, double setPoint, double maxGain, double rate, double initGain) {
    auto* a = as_block<FastAgcBlock>(h, "a FastAGC");
    if (!a) return SDRGPU_EARG;
    a->set(setPoint, maxGain, rate, initGain);
    return SDRGPU_OK;
}
extern "C" int sdrgpu_fast_agc_set_gain(sdrgpu_block* h, double gain) {
    auto* a = as_block<FastAgcBlock>(h, "a FastAGC");
    if (!a) return SDRGPU_EARG;
    a->set_gain(gain);
    return SDRGPU_OK;
}
extern "C" int sdrgpu_fast_agc_get_gain(sdrgpu_block* h, float* gain) {
    auto* a = as_block<FastAgcBlock>(h, "a FastAGC");
    if (!a || !gain) { if (a) set_error("fast_agc_get_gain: null pointer"); return SDRGPU_EARG; }
    SDRGPU_CHECK(enter_block(h, !a->p.hasGain));   // (UI-rate query: waits for the block's queued work)
    return a->get_gain(gain);
}

extern "C" int sdrgpu_costas_create(sdrgpu_block** h, int device, int order, double bandwidth, double initPhase, double initFreq,
                                    double minFreq, double maxFreq) {
    if (!h) { set_error("costas_create: null handle pointer"); return SDRGPU_EARG; }
    if (!costas_args_ok(order, bandwidth, initPhase, initFreq, minFreq, maxFreq)) return SDRGPU_EARG;   // before the device is touched
    SDRGPU_SET_DEVICE(device);
    auto* c = new CostasBlock();
    return publish_block(h, c, c->setup(device, order, bandwidth, initPhase, initFreq, minFreq, maxFreq));
}
extern "C" int sdrgpu_costas_set_bandwidth(sdrgpu_block* h, double bandwidth) {
    auto* c = as_block<CostasBlock>(h, "a Costas loop");
    if (!c || !std::isfinite(bandwidth)) return SDRGPU_EARG;
    critically_damped(bandwidth, &c->p.pcl.alpha, &c->p.pcl.beta);
    return SDRGPU_OK;
}
extern "C" int sdrgpu_costas_set_freq_limits(sdrgpu_block* h, double minFreq, double maxFreq) {
    auto* c = as_block<CostasBlock>(h, "a Costas loop");
    if (!c) return SDRGPU_EARG;
    if (!costas_limits_ok(minFreq, maxFreq)) { set_error("costas: bad frequency limits"); return SDRGPU_EARG; }
    c->p.pcl.minFreq = (float)minFreq;
    c->p.pcl.maxFreq = (float)maxFreq;
    c->p.clampNow = 1;
    return SDRGPU_OK;
}

// loop::PLL / loop::CarrierTrackingPLL / loop::MeteorCostas: sdrgpu_costas_set_bandwidth and _set_freq_limits are
// their setBandwidth and setFrequencyLimits too (all four are PLLs, pll.h:27-53)
static int pll_create(sdrgpu_block** h, int device, bool derotate, double bandwidth, double initPhase, double initFreq,
                      double minFreq, double maxFreq) {
    if (!h) { set_error("pll_create: null handle pointer"); return SDRGPU_EARG; }
    if (!costas_args_ok(4, bandwidth, initPhase, initFreq, minFreq, maxFreq)) return SDRGPU_EARG;   // before the device is touched
    SDRGPU_SET_DEVICE(device);
    auto* c = new PllBlock();
    c->derotate = derotate;
    return publish_block(h, c, c->setup(device, 4, bandwidth, initPhase, initFreq, minFreq, maxFreq));
}
extern "C" int sdrgpu_pll_create(sdrgpu_block** h, int device, double bandwidth, double initPhase, double initFreq, double minFreq,
                                 double maxFreq) {
    return pll_create(h, device, false, bandwidth, initPhase, initFreq, minFreq, maxFreq);
}
extern "C" int sdrgpu_carrier_pll_create(sdrgpu_block** h, int device, double bandwidth, double initPhase, double initFreq,
                                         double minFreq, double maxFreq) {
    return pll_create(h, device, true, bandwidth, initPhase, initFreq, minFreq, maxFreq);
}
extern "C" int sdrgpu_meteor_costas_create(sdrgpu_block** h, int device, double bandwidth, int brokenModulation, double initPhase,
                                           double initFreq, double minFreq, double maxFreq) {
    if (!h) { set_error("meteor_costas_create: null handle pointer"); return SDRGPU_EARG; }
    if (!costas_args_ok(4, bandwidth, initPhase, initFreq, minFreq, maxFreq)) return SDRGPU_EARG;   // before the device is touched
    SDRGPU_SET_DEVICE(device);
    auto* c = new MeteorCostasBlock();
    return publish_block(h, c, c->setup(device, bandwidth, brokenModulation, 0, initPhase, initFreq, minFreq, maxFreq));
}
// setBrokenModulation (meteor_costas.h:18-22, meteor_demod.h:127-131): from the next call, the loop state is kept
extern "C" int sdrgpu_meteor_costas_set_broken_modulation(sdrgpu_block* h, int enabled) {
    auto* c = as_block<MeteorCostasBlock>(h, "a MeteorCostas loop");
    if (!c) return SDRGPU_EARG;
    c->broken = enabled ? 1 : 0;
    return SDRGPU_OK;
}
extern "C" int sdrgpu_meteor_set_broken_modulation(sdrgpu_block* h, int enabled) {
    return sdrgpu_meteor_costas_set_broken_modulation(h, enabled);
}
// setOQPSK (meteor_demod.h:133-137): from the next call; lastI keeps the value it had when the stagger last ran
extern "C" int sdrgpu_meteor_set_oqpsk(sdrgpu_block* h, int enabled) {
    auto* c = find_kid<MeteorCostasBlock>(h, false);
    if (!c) { set_error("not a Meteor demodulator"); return SDRGPU_EARG; }
    c->oqpsk = enabled ? 1 : 0;
    return SDRGPU_OK;
}

extern "C" int sdrgpu_mm_create(sdrgpu_block** h, int device, int dtype, double omega, double omegaGain, double muGain,
                                double omegaRelLimit, int interpPhases, int interpTaps) {
    if (!h || !real_or_complex(dtype)) { set_error("mm_create: bad argument"); return SDRGPU_EARG; }
    if (!mm_args_ok(omega, omegaGain, muGain, omegaRelLimit, interpPhases, interpTaps)) return SDRGPU_EARG;   // before the device is touched
    SDRGPU_SET_DEVICE(device);
    auto* m = new MmBlock();
    return publish_block(h, m, m->setup(device, dtype, MmEpilogue::Soft, 1, omega, omegaGain, muGain, omegaRelLimit, interpPhases, interpTaps));
}
// the MM setters: on an MM handle, or on a PSK / GFSK / RDS handle (its last block)
static int mm_set(sdrgpu_block* h, double omega, double omegaGain, double muGain, double rel, bool newOmega) {
    MmBlock* m = mm_of(h);
    if (!m) return SDRGPU_EARG;
    if (!mm_params_ok(omega, omegaGain, muGain, rel)) {
        set_error("mm: omega * (1 - omegaRelLimit) - muGain must be >= 1 (an output per input sample at most)");
        return SDRGPU_EARG;
    }
    const bool newLimits = rel != m->rel;
    m->omega = omega; m->omegaGain = omegaGain; m->muGain = muGain; m->rel = rel;
    m->set_pcl();
    if (newOmega) m->p.setOmega = 1;
    if (newLimits) m->p.clampNow = 1;
    return SDRGPU_OK;
}
extern "C" int sdrgpu_mm_set_omega(sdrgpu_block* h, double omega) {
    MmBlock* m = mm_of(h);
    return m ? mm_set(h, omega, m->omegaGain, m->muGain, m->rel, true) : SDRGPU_EARG;
}
extern "C" int sdrgpu_mm_set_gains(sdrgpu_block* h, double omegaGain, double muGain) {
    MmBlock* m = mm_of(h);
    return m ? mm_set(h, m->omega, omegaGain, muGain, m->rel, false) : SDRGPU_EARG;
}
extern "C" int sdrgpu_mm_set_omega_rel_limit(sdrgpu_block* h, double omegaRelLimit) {
    MmBlock* m = mm_of(h);
    if (!m) return SDRGPU_EARG;
    const int rc = mm_set(h, m->omega, m->omegaGain, m->muGain, omegaRelLimit, false);
    if (rc >= 0) m->p.clampNow = 1;   // setFreqLimits clamps even where the limit is unchanged
    return rc;
}

extern "C" int sdrgpu_binary_slicer_create(sdrgpu_block** h, int device) {
    if (!h) { set_error("binary_slicer_create: null handle pointer"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    auto* b = new SlicerBlock();
    b->device = device;
    b->in_dtype = SDRGPU_F32;
    b->out_dtype = SDRGPU_U8;
    return publish_block(h, b, SDRGPU_OK);
}
extern "C" int sdrgpu_differential_decoder_create(sdrgpu_block** h, int device, int modulus, int initSym) {
    if (!h || modulus < 1 || modulus > 255 || initSym < 0 || initSym > 255) { set_error("differential_decoder_create: bad argument"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    auto* d = new DiffDecoderBlock();
    return publish_block(h, d, d->setup(device, modulus, initSym));
}

extern "C" int sdrgpu_psk_create(sdrgpu_block** h, int device, int order, double symbolrate, double samplerate, int rrcTapCount,
                                 double rrcBeta, double agcRate, double costasBandwidth, double omegaGain, double muGain,
                                 double omegaRelLimit) {
    if (!h || !(symbolrate > 0) || !(samplerate > 0)) { set_error("psk_create: bad argument"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    Block* c = chain_new(device, SDRGPU_C64, SDRGPU_C64);
    int rc;
    Block* b = make_rrc_fir(device, SDRGPU_C64, rrcTapCount, rrcBeta, symbolrate, samplerate, &rc);
    rc = append_owned(c, b, rc);
    if (rc >= 0) { b = make_fast_agc(device, SDRGPU_C64, 1.0, 10e6, agcRate, 1.0, &rc); rc = append_owned(c, b, rc); }
    const double PI = 3.1415926535f;   // FL_M_PI, the default frequency limits (pll.h:15)
    if (rc >= 0) { b = make_costas(device, order, costasBandwidth, 0.0, 0.0, -PI, PI, &rc); rc = append_owned(c, b, rc); }
    if (rc >= 0) {
        b = make_mm(device, SDRGPU_C64, MmEpilogue::Soft, 1, samplerate / symbolrate, omegaGain, muGain, omegaRelLimit, 128, 8, &rc);
        rc = append_owned(c, b, rc);
    }
    return publish_block(h, c, rc);
}

// demod::Meteor (meteor_demod.h:24-43, 150-167). Every argument is checked before the device is touched.
extern "C" int sdrgpu_meteor_create(sdrgpu_block** h, int device, double symbolrate, double samplerate, int rrcTapCount,
                                    double rrcBeta, double agcRate, double costasBandwidth, int brokenModulation, int oqpsk,
                                    double omegaGain, double muGain, double omegaRelLimit) {
    if (!h || !(symbolrate > 0) || !(samplerate > 0)) { set_error("meteor_create: bad argument"); return SDRGPU_EARG; }
    const double PI = 3.1415926535f;   // FL_M_PI, the default frequency limits (meteor_costas.h:13)
    std::vector<float> t;
    SDRGPU_CHECK(design_taps(t, taps_root_raised_cosine, rrcTapCount, rrcBeta, samplerate / symbolrate));
    if (!costas_args_ok(4, costasBandwidth, 0.0, 0.0, -PI, PI) ||
        !mm_args_ok(samplerate / symbolrate, omegaGain, muGain, omegaRelLimit, 128, 8))
        return SDRGPU_EARG;
    SDRGPU_SET_DEVICE(device);
    Block* c = chain_new(device, SDRGPU_C64, SDRGPU_C64);
    int rc;
    auto* f = new OrderedFirBlock();   // :31-32
    Block* b = f;
    rc = append_owned(c, f, f->setup(device, t.data(), (int)t.size()));
    if (rc >= 0) { b = make_fast_agc(device, SDRGPU_C64, 1.0, 10e6, agcRate, 1.0, &rc); rc = append_owned(c, b, rc); }   // :33
    if (rc >= 0) {   // :34, and the stagger of :155-164 on its output
        auto* m = new MeteorCostasBlock();
        rc = append_owned(c, m, m->setup(device, costasBandwidth, brokenModulation, oqpsk, 0.0, 0.0, -PI, PI));
    }
    if (rc >= 0) {   // :35
        b = make_mm(device, SDRGPU_C64, MmEpilogue::Soft, 1, samplerate / symbolrate, omegaGain, muGain, omegaRelLimit, 128, 8, &rc);
        rc = append_owned(c, b, rc);
    }
    return publish_block(h, c, rc);
}

extern "C" int sdrgpu_gfsk_create(sdrgpu_block** h, int device, double symbolrate, double samplerate, double deviation,
                                  int rrcTapCount, double rrcBeta, double omegaGain, double muGain, double omegaRelLimit) {
    if (!h || !(symbolrate > 0) || !(samplerate > 0)) { set_error("gfsk_create: bad argument"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    Block* c = chain_new(device, SDRGPU_C64, SDRGPU_F32);
    int rc;
    Block* b = make_quad_block(device, hz_to_rads(deviation, samplerate), &rc);   // Quadrature::init(in, deviation, samplerate)
    rc = append_owned(c, b, rc);
    if (rc >= 0) { b = make_rrc_fir(device, SDRGPU_F32, rrcTapCount, rrcBeta, symbolrate, samplerate, &rc); rc = append_owned(c, b, rc); }
    if (rc >= 0) {
        b = make_mm(device, SDRGPU_F32, MmEpilogue::Soft, 1, samplerate / symbolrate, omegaGain, muGain, omegaRelLimit, 128, 8, &rc);
        rc = append_owned(c, b, rc);
    }
    return publish_block(h, c, rc);
}

// wfm.h:57-68
extern "C" int sdrgpu_rds_create(sdrgpu_block** h, int device) {
    if (!h) { set_error("rds_create: null handle pointer"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(device);
    Block* c = chain_new(device, SDRGPU_C64, SDRGPU_U8);
    int rc;
    const double PI = 3.1415926535f;
    Block* b = make_fast_agc(device, SDRGPU_C64, 1.0, 1e6, 0.1, 1.0, &rc);
    rc = append_owned(c, b, rc);
    if (rc >= 0) { b = make_costas(device, 2, 0.005f, 0.0, 0.0, -PI, PI, &rc); rc = append_owned(c, b, rc); }
    if (rc >= 0) {
        const int n = taps_band_pass_c(0.0, 2375.0, 100.0, 5000.0, 0, nullptr);
        std::vector<float> t(2 * (size_t)std::max(n, 1));
        rc = n < 1 ? (n < 0 ? n : SDRGPU_EARG) : taps_band_pass_c(0.0, 2375.0, 100.0, 5000.0, 0, t.data());
        if (rc >= 0) { b = make_fir_block(device, SDRGPU_C64, SDRGPU_C64, t.data(), n, 1, false, &rc); rc = append_owned(c, b, rc); }
    }
    if (rc >= 0) {
        const double w = hz_to_rads(2375.0 / 2.0, 5000.0);
        b = make_costas(device, 2, 0.01, 0.0, w, w - (w * 0.1), w + (w * 0.1), &rc);
        rc = append_owned(c, b, rc);
    }
    if (rc >= 0) {   // ComplexToReal in the MM kernel's staging; BinarySlicer and DifferentialDecoder(2) in its epilogue
        b = make_mm(device, SDRGPU_F32, MmEpilogue::DiffBits, 2, 5000.0 / (2375.0 / 2.0), 1e-6, 0.01, 0.01, 128, 8, &rc);
        rc = append_owned(c, b, rc);
    }
    return publish_block(h, c, rc);
}
extern "C" int sdrgpu_rds_symbols_dev(sdrgpu_block* h, const float** out, int* n) {
    MmBlock* m = mm_of(h);
    if (!m || m->epi != MmEpilogue::DiffBits) { set_error("not an RDS block"); return SDRGPU_EARG; }
    if (out) *out = m->soft.as<float>();
    if (n) *n = m->lastCount;
    return m->lastCount;
}
