// GPU-backed dsp::demod::Meteor -- drop-in for decoder_modules/meteor_demodulator/src/meteor_demod.h:
// FIR(rootRaisedCosine) -> FastAGC(1, 10e6, agcRate) -> MeteorCostas -> the OQPSK stagger -> MM<complex_t> as one
// device chain (sdrgpu_meteor_create, sdrpp_amd/csrc/symsync.hip). The AGC, Costas, MM, broken-modulation and OQPSK
// setters reach the running chain; setSymbolrate / setSamplerate / setRRCParams rebuild it (new taps and omega), so
// the loops restart there as after reset(), and the stagger's carry starts again at 0 (one sample's Q).
#pragma once
#include <dsp/processor.h>
#include <dsp/sdrgpu_handle.h>
#include "meteor_costas.h"

namespace dsp::demod {
class Meteor : public Processor<complex_t, complex_t> {
    using base_type = Processor<complex_t, complex_t>;
public:
    Meteor() {}
    Meteor(stream<complex_t>* in, double symbolrate, double samplerate, int rrcTapCount, double rrcBeta, double agcRate, double costasBandwidth, bool brokenModulation, bool oqpsk, double omegaGain, double muGain, double omegaRelLimit = 0.01) {
        init(in, symbolrate, samplerate, rrcTapCount, rrcBeta, agcRate, costasBandwidth, brokenModulation, oqpsk, omegaGain, muGain);   // (meteor_demod.h:15 drops omegaRelLimit too)
    }
    void init(stream<complex_t>* in, double symbolrate, double samplerate, int rrcTapCount, double rrcBeta, double agcRate, double costasBandwidth, bool brokenModulation, bool oqpsk, double omegaGain, double muGain, double omegaRelLimit = 0.01) {
        _symbolrate = symbolrate; _samplerate = samplerate; _rrcTapCount = rrcTapCount; _rrcBeta = rrcBeta;
        _agcRate = agcRate; _costasBandwidth = costasBandwidth; _broken = brokenModulation; _oqpsk = oqpsk;
        _omegaGain = omegaGain; _muGain = muGain; _omegaRelLimit = omegaRelLimit;
        create();
        base_type::init(in);
    }
    void setSymbolrate(double symbolrate) { _symbolrate = symbolrate; rebuild(); }
    void setSamplerate(double samplerate) { _samplerate = samplerate; rebuild(); }
    void setRRCParams(int rrcTapCount, double rrcBeta) { _rrcTapCount = rrcTapCount; _rrcBeta = rrcBeta; rebuild(); }
    void setRRCTapCount(int rrcTapCount) { setRRCParams(rrcTapCount, _rrcBeta); }
    void setRRCBeta(int rrcBeta) { setRRCParams(_rrcTapCount, rrcBeta); }
    void setAGCRate(double agcRate) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        _agcRate = agcRate;
        gpu::ok(sdrgpu_fast_agc_set(_h.h, 1.0, 10e6, agcRate, 1.0), "meteor_set_agc_rate");
    }
    void setCostasBandwidth(double bandwidth) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        _costasBandwidth = bandwidth;
        gpu::ok(sdrgpu_costas_set_bandwidth(_h.h, bandwidth), "meteor_set_costas_bandwidth");
    }
    void setMMParams(double omegaGain, double muGain, double omegaRelLimit = 0.01) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        if (gpu::ok(sdrgpu_mm_set_gains(_h.h, omegaGain, muGain), "meteor_set_mm_gains")) { _omegaGain = omegaGain; _muGain = muGain; }
        if (gpu::ok(sdrgpu_mm_set_omega_rel_limit(_h.h, omegaRelLimit), "meteor_set_omega_rel_limit")) _omegaRelLimit = omegaRelLimit;
    }
    void setOmegaGain(double omegaGain) { setMMParams(omegaGain, _muGain, _omegaRelLimit); }
    void setMuGain(double muGain) { setMMParams(_omegaGain, muGain, _omegaRelLimit); }
    void setOmegaRelLimit(double omegaRelLimit) { setMMParams(_omegaGain, _muGain, omegaRelLimit); }
    void setBrokenModulation(bool enabled) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        _broken = enabled;
        gpu::ok(sdrgpu_meteor_set_broken_modulation(_h.h, enabled ? 1 : 0), "meteor_set_broken_modulation");
    }
    void setOQPSK(bool enabled) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        _oqpsk = enabled;
        gpu::ok(sdrgpu_meteor_set_oqpsk(_h.h, enabled ? 1 : 0), "meteor_set_oqpsk");
    }
    void reset() {   // the four blocks; the stagger's carry stays (meteor_demod.h:139-148)
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        base_type::tempStop();
        gpu::ok(sdrgpu_block_reset(_h.h), "meteor_reset");
        base_type::tempStart();
    }
    inline int process(int count, const complex_t* in, complex_t* out) { return _h.process(in, count, out, "meteor"); }
    int run() override {
        int count = base_type::_in->read();
        if (count < 0) return -1;
        int outCount = process(count, base_type::_in->readBuf, base_type::out.writeBuf);
        base_type::_in->flush();
        if (outCount < 0) return -1;
        if (outCount) {   // swap if some data was generated (meteor_demod.h:176-179)
            if (!base_type::out.swap(outCount)) return -1;
        }
        return outCount;
    }

protected:
    void create() {
        sdrgpu_block* h = nullptr;
        gpu::ok(sdrgpu_meteor_create(&h, _h.bind(gpu::device()), _symbolrate, _samplerate, _rrcTapCount, _rrcBeta, _agcRate, _costasBandwidth,
                                     _broken ? 1 : 0, _oqpsk ? 1 : 0, _omegaGain, _muGain, _omegaRelLimit), "meteor_create");
        _h.reset(h);
    }
    void rebuild() {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        base_type::tempStop();
        create();
        base_type::tempStart();
    }
    double _symbolrate = 1, _samplerate = 1, _rrcBeta = 0, _agcRate = 0, _costasBandwidth = 0, _omegaGain = 0, _muGain = 0, _omegaRelLimit = 0.01;
    int _rrcTapCount = 1;
    bool _broken = false, _oqpsk = false;
    gpu::Handle _h;
};
}  // namespace dsp::demod
