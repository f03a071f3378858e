// GPU-backed dsp::demod::GFSK -- drop-in for core/src/dsp/demod/gfsk.h: Quadrature(deviation) ->
// FIR(rootRaisedCosine) -> MM<float> as one device chain (sdrgpu_gfsk_create,
// sdrpp_amd/csrc/symsync.hip). The MM setters reach the running chain; setSymbolrate / setSamplerate /
// setDeviation / setRRCParams rebuild it, so the loop restarts there as after reset().
#pragma once
#include "../processor.h"
#include "../sdrgpu_handle.h"

namespace dsp::demod {
class GFSK : public Processor<complex_t, float> {
    using base_type = Processor<complex_t, float>;
public:
    GFSK() {}
    GFSK(stream<complex_t>* in, double symbolrate, double samplerate, double deviation, int rrcTapCount, double rrcBeta, double omegaGain, double muGain, double omegaRelLimit = 0.01) {
        init(in, symbolrate, samplerate, deviation, rrcTapCount, rrcBeta, omegaGain, muGain);   // (gfsk.h:15 drops omegaRelLimit too)
    }
    void init(stream<complex_t>* in, double symbolrate, double samplerate, double deviation, int rrcTapCount, double rrcBeta, double omegaGain, double muGain, double omegaRelLimit = 0.01) {
        _symbolrate = symbolrate; _samplerate = samplerate; _deviation = deviation; _rrcTapCount = rrcTapCount; _rrcBeta = rrcBeta;
        _omegaGain = omegaGain; _muGain = muGain; _omegaRelLimit = omegaRelLimit;
        create();
        base_type::init(in);
    }
    void setSymbolrate(double symbolrate) { _symbolrate = symbolrate; rebuild(); }
    void setSamplerate(double samplerate) { _samplerate = samplerate; rebuild(); }
    void setDeviation(double deviation) { _deviation = deviation; rebuild(); }
    void setRRCParams(int rrcTapCount, double rrcBeta) { _rrcTapCount = rrcTapCount; _rrcBeta = rrcBeta; rebuild(); }
    void setRRCTapCount(int rrcTapCount) { setRRCParams(rrcTapCount, _rrcBeta); }
    void setRRCBeta(int rrcBeta) { setRRCParams(_rrcTapCount, rrcBeta); }
    void setMMParams(double omegaGain, double muGain, double omegaRelLimit = 0.01) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        if (gpu::ok(sdrgpu_mm_set_gains(_h.h, omegaGain, muGain), "gfsk_set_mm_gains")) { _omegaGain = omegaGain; _muGain = muGain; }
        if (gpu::ok(sdrgpu_mm_set_omega_rel_limit(_h.h, omegaRelLimit), "gfsk_set_omega_rel_limit")) _omegaRelLimit = omegaRelLimit;
    }
    void setOmegaGain(double omegaGain) { setMMParams(omegaGain, _muGain, _omegaRelLimit); }
    void setMuGain(double muGain) { setMMParams(_omegaGain, muGain, _omegaRelLimit); }
    void setOmegaRelLimit(double omegaRelLimit) { setMMParams(_omegaGain, _muGain, omegaRelLimit); }
    void reset() {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        base_type::tempStop();
        gpu::ok(sdrgpu_block_reset(_h.h), "gfsk_reset");
        base_type::tempStart();
    }
    inline int process(int count, complex_t* in, float* out) { return _h.process(in, count, out, "gfsk"); }
    int run() override {
        int count = base_type::_in->read();
        if (count < 0) return -1;
        int outCount = process(count, base_type::_in->readBuf, base_type::out.writeBuf);
        base_type::_in->flush();
        if (outCount < 0) return -1;
        if (outCount) {   // swap if some data was generated (gfsk.h:143-147)
            if (!base_type::out.swap(outCount)) return -1;
        }
        return outCount;
    }

protected:
    void create() {
        sdrgpu_block* h = nullptr;
        gpu::ok(sdrgpu_gfsk_create(&h, _h.bind(gpu::device()), _symbolrate, _samplerate, _deviation, _rrcTapCount, _rrcBeta, _omegaGain,
                                   _muGain, _omegaRelLimit), "gfsk_create");
        _h.reset(h);
    }
    void rebuild() {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        base_type::tempStop();
        create();
        base_type::tempStart();
    }
    double _symbolrate = 1, _samplerate = 1, _deviation = 0, _rrcBeta = 0, _omegaGain = 0, _muGain = 0, _omegaRelLimit = 0.01;
    int _rrcTapCount = 1;
    gpu::Handle _h;
};
}  // namespace dsp::demod
