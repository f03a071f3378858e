// GPU-backed dsp::loop::MeteorCostas -- drop-in for decoder_modules/meteor_demodulator/src/meteor_costas.h. The
// loop runs on the device in the reference's operation order (meteor_costas.h:24-56 over pll.h:15-62,
// phase_control_loop.h:58-85; sdrpp_amd/csrc/symsync.hip). It derives from Processor<complex_t, complex_t>
// directly, as the overlay's loop/costas.h does. init and the setters are PLL's (loop/pll.h:15-62) and
// setBrokenModulation; the constructor passes (initFreq, initPhase) to init in that order, as meteor_costas.h:11 does.
#pragma once
#include <dsp/processor.h>
#include <dsp/math/constants.h>
#include <dsp/sdrgpu_handle.h>

namespace dsp::loop {
class MeteorCostas : public Processor<complex_t, complex_t> {
    using base_type = Processor<complex_t, complex_t>;
public:
    MeteorCostas() {}
    MeteorCostas(stream<complex_t>* in, double bandwidth, bool brokenModulation, double initPhase = 0.0, double initFreq = 0.0, double minFreq = -FL_M_PI, double maxFreq = FL_M_PI) {
        init(in, bandwidth, brokenModulation, initFreq, initPhase, minFreq, maxFreq);
    }
    void init(stream<complex_t>* in, double bandwidth, bool brokenModulation, double initPhase = 0.0, double initFreq = 0.0, double minFreq = -FL_M_PI, double maxFreq = FL_M_PI) {
        _bandwidth = bandwidth; _broken = brokenModulation; _initPhase = initPhase; _initFreq = initFreq; _minFreq = minFreq; _maxFreq = maxFreq;
        create();
        base_type::init(in);
    }
    void setBrokenModulation(bool enabled) {   // the running loop keeps its state (meteor_costas.h:18-22)
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        _broken = enabled;
        gpu::ok(sdrgpu_meteor_costas_set_broken_modulation(_h.h, enabled ? 1 : 0), "meteor_costas_set_broken_modulation");
    }
    void setBandwidth(double bandwidth) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        _bandwidth = bandwidth;
        gpu::ok(sdrgpu_costas_set_bandwidth(_h.h, bandwidth), "meteor_costas_set_bandwidth");
    }
    // the initial phase / frequency are what reset() goes back to (pll.h:37-47): kept here, reset() rebuilds with them
    void setInitialPhase(double initPhase) { std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx); _initPhase = initPhase; }
    void setInitialFreq(double initFreq) { std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx); _initFreq = initFreq; }
    void setFrequencyLimits(double minFreq, double maxFreq) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        _minFreq = minFreq; _maxFreq = maxFreq;
        gpu::ok(sdrgpu_costas_set_freq_limits(_h.h, minFreq, maxFreq), "meteor_costas_set_freq_limits");
    }
    void reset() {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        base_type::tempStop();
        create();
        base_type::tempStart();
    }
    inline int process(int count, complex_t* in, complex_t* out) { return _h.process(in, count, out, "meteor_costas"); }
    int run() override {
        int count = base_type::_in->read();
        if (count < 0) return -1;
        int n = process(count, base_type::_in->readBuf, base_type::out.writeBuf);
        base_type::_in->flush();
        if (n < 0 || !base_type::out.swap(count)) return -1;
        return count;
    }

protected:
    void create() {
        sdrgpu_block* h = nullptr;
        gpu::ok(sdrgpu_meteor_costas_create(&h, _h.bind(gpu::device()), _bandwidth, _broken ? 1 : 0, _initPhase, _initFreq, _minFreq, _maxFreq),
                "meteor_costas_create");
        _h.reset(h);
    }
    double _bandwidth = 0, _initPhase = 0, _initFreq = 0, _minFreq = -FL_M_PI, _maxFreq = FL_M_PI;
    bool _broken = false;
    gpu::Handle _h;
};
}  // namespace dsp::loop
