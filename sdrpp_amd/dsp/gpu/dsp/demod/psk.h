// GPU-backed dsp::demod::PSK<ORDER> -- drop-in for core/src/dsp/demod/psk.h: FIR(rootRaisedCosine) ->
// FastAGC(1, 10e6, agcRate) -> Costas<ORDER> -> MM<complex_t> as one device chain
// (sdrgpu_psk_create, sdrpp_amd/csrc/symsync.hip). The AGC, Costas and MM setters reach the running
// chain; setSymbolrate / setSamplerate / setRRCParams rebuild it (new taps and omega), so the loops
// restart there as after reset().
#pragma once
#include "../processor.h"
#include "../sdrgpu_handle.h"

namespace dsp::demod {
template <int ORDER>
class PSK : public Processor<complex_t, complex_t> {
    static_assert(ORDER == 2 || ORDER == 4 || ORDER == 8, "Invalid costas order");
    using base_type = Processor<complex_t, complex_t>;
public:
    PSK() {}
    PSK(stream<complex_t>* in, double symbolrate, double samplerate, int rrcTapCount, double rrcBeta, double agcRate, double costasBandwidth, double omegaGain, double muGain, double omegaRelLimit = 0.01) {
        init(in, symbolrate, samplerate, rrcTapCount, rrcBeta, agcRate, costasBandwidth, omegaGain, muGain);   // (psk.h:16 drops omegaRelLimit too)
    }
    void init(stream<complex_t>* in, double symbolrate, double samplerate, int rrcTapCount, double rrcBeta, double agcRate, double costasBandwidth, double omegaGain, double muGain, double omegaRelLimit = 0.01) {
        _symbolrate = symbolrate; _samplerate = samplerate; _rrcTapCount = rrcTapCount; _rrcBeta = rrcBeta;
        _agcRate = agcRate; _costasBandwidth = costasBandwidth; _omegaGain = omegaGain; _muGain = muGain; _omegaRelLimit = omegaRelLimit;
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
        gpu::ok(sdrgpu_fast_agc_set(_h.h, 1.0, 10e6, agcRate, 1.0), "psk_set_agc_rate");
    }
    void setCostasBandwidth(double bandwidth) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        _costasBandwidth = bandwidth;
        gpu::ok(sdrgpu_costas_set_bandwidth(_h.h, bandwidth), "psk_set_costas_bandwidth");
    }
    void setMMParams(double omegaGain, double muGain, double omegaRelLimit = 0.01) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        if (gpu::ok(sdrgpu_mm_set_gains(_h.h, omegaGain, muGain), "psk_set_mm_gains")) { _omegaGain = omegaGain; _muGain = muGain; }
        if (gpu::ok(sdrgpu_mm_set_omega_rel_limit(_h.h, omegaRelLimit), "psk_set_omega_rel_limit")) _omegaRelLimit = omegaRelLimit;
    }
    void setOmegaGain(double omegaGain) { setMMParams(omegaGain, _muGain, _omegaRelLimit); }
    void setMuGain(double muGain) { setMMParams(_omegaGain, muGain, _omegaRelLimit); }
    void setOmegaRelLimit(double omegaRelLimit) { setMMParams(_omegaGain, _muGain, omegaRelLimit); }
    void reset() {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        base_type::tempStop();
        gpu::ok(sdrgpu_block_reset(_h.h), "psk_reset");
        base_type::tempStart();
    }
    inline int process(int count, const complex_t* in, complex_t* out) { return _h.process(in, count, out, "psk"); }
    int run() override {
        int count = base_type::_in->read();
        if (count < 0) return -1;
        int outCount = process(count, base_type::_in->readBuf, base_type::out.writeBuf);
        base_type::_in->flush();
        if (outCount < 0) return -1;
        if (outCount) {   // swap if some data was generated (psk.h:151-155)
            if (!base_type::out.swap(outCount)) return -1;
        }
        return outCount;
    }

protected:
    void create() {
        sdrgpu_block* h = nullptr;
        gpu::ok(sdrgpu_psk_create(&h, _h.bind(gpu::device()), ORDER, _symbolrate, _samplerate, _rrcTapCount, _rrcBeta, _agcRate,
                                  _costasBandwidth, _omegaGain, _muGain, _omegaRelLimit), "psk_create");
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
    gpu::Handle _h;
};
}  // namespace dsp::demod
