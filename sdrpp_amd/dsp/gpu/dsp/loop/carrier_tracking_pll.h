// GPU-backed dsp::loop::CarrierTrackingPLL -- drop-in for core/src/dsp/loop/carrier_tracking_pll.h. The loop
// runs on the device in the reference's operation order (carrier_tracking_pll.h:14-20 over pll.h:15-62,
// phase_control_loop.h:58-85; sdrpp_amd/csrc/symsync.hip). It derives from Processor<complex_t, complex_t>
// directly: the host PLL it derives from in the reference has no state left to share (there is no overlay
// loop/pll.h: INTEGRATION.md says why). init and the setters are PLL's (loop/pll.h:15-62); the constructor
// passes (initFreq, initPhase) to init in that order, as carrier_tracking_pll.h:10-12 does.
#pragma once
#include "../processor.h"
#include "../math/constants.h"
#include "../sdrgpu_handle.h"

namespace dsp::loop {
class CarrierTrackingPLL : public Processor<complex_t, complex_t> {
    using base_type = Processor<complex_t, complex_t>;
public:
    CarrierTrackingPLL() {}
    CarrierTrackingPLL(stream<complex_t>* in, double bandwidth, double initPhase = 0.0, double initFreq = 0.0, double minFreq = -FL_M_PI, double maxFreq = FL_M_PI) {
        init(in, bandwidth, initFreq, initPhase, minFreq, maxFreq);
    }
    void init(stream<complex_t>* in, double bandwidth, double initPhase = 0.0, double initFreq = 0.0, double minFreq = -FL_M_PI, double maxFreq = FL_M_PI) {
        _bandwidth = bandwidth; _initPhase = initPhase; _initFreq = initFreq; _minFreq = minFreq; _maxFreq = maxFreq;
        create();
        base_type::init(in);
    }
    void setBandwidth(double bandwidth) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        _bandwidth = bandwidth;
        gpu::ok(sdrgpu_costas_set_bandwidth(_h.h, bandwidth), "carrier_pll_set_bandwidth");
    }
    // the initial phase / frequency are what reset() goes back to (pll.h:37-47): kept here, reset() rebuilds with them
    void setInitialPhase(double initPhase) { std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx); _initPhase = initPhase; }
    void setInitialFreq(double initFreq) { std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx); _initFreq = initFreq; }
    void setFrequencyLimits(double minFreq, double maxFreq) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        _minFreq = minFreq; _maxFreq = maxFreq;
        gpu::ok(sdrgpu_costas_set_freq_limits(_h.h, minFreq, maxFreq), "carrier_pll_set_freq_limits");
    }
    void reset() {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        base_type::tempStop();
        create();
        base_type::tempStart();
    }
    inline int process(int count, complex_t* in, complex_t* out) { return _h.process(in, count, out, "carrier_pll"); }
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
        gpu::ok(sdrgpu_carrier_pll_create(&h, _h.bind(gpu::device()), _bandwidth, _initPhase, _initFreq, _minFreq, _maxFreq), "carrier_pll_create");
        _h.reset(h);
    }
    double _bandwidth = 0, _initPhase = 0, _initFreq = 0, _minFreq = -FL_M_PI, _maxFreq = FL_M_PI;
    gpu::Handle _h;
};
}  // namespace dsp::loop
