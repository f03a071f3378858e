// GPU-backed dsp::loop::FastAGC<T> -- drop-in for core/src/dsp/loop/fast_agc.h (T = float or complex_t).
// The recurrence runs on the device bit-identically to fast_agc.h:60-79 (sdrpp_amd/csrc/symsync.hip);
// the setters keep the gain, setGain is applied at the next process().
#pragma once
#include <type_traits>
#include "../processor.h"
#include "../sdrgpu_handle.h"

namespace dsp::loop {
template <class T>
class FastAGC : public Processor<T, T> {
    using base_type = Processor<T, T>;
    static_assert(std::is_same_v<T, float> || std::is_same_v<T, complex_t>, "FastAGC<T>: T = float or complex_t");
public:
    FastAGC() {}
    FastAGC(stream<T>* in, double setPoint, double maxGain, double rate, double initGain = 1.0) { init(in, setPoint, maxGain, rate, initGain); }
    void init(stream<T>* in, double setPoint, double maxGain, double rate, double initGain = 1.0) {
        _setPoint = setPoint; _maxGain = maxGain; _rate = rate; _initGain = initGain;
        sdrgpu_block* h = nullptr;
        gpu::ok(sdrgpu_fast_agc_create(&h, _h.bind(gpu::device()), std::is_same_v<T, complex_t> ? SDRGPU_C64 : SDRGPU_F32, setPoint,
                                       maxGain, rate, initGain), "fast_agc_create");
        _h.reset(h);
        base_type::init(in);
    }
    void setSetPoint(double setPoint) { _setPoint = setPoint; params(); }
    void setMaxGain(double maxGain) { _maxGain = maxGain; params(); }
    void setRate(double rate) { _rate = rate; params(); }
    void setInitGain(double initGain) { _initGain = initGain; params(); }
    void setGain(double gain) { std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx); gpu::ok(sdrgpu_fast_agc_set_gain(_h.h, gain), "fast_agc_set_gain"); }
    void reset() { std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx); gpu::ok(sdrgpu_block_reset(_h.h), "fast_agc_reset"); }
    inline int process(int count, T* in, T* out) { return _h.process(in, count, out, "fast_agc"); }
    int run() override {
        int count = base_type::_in->read();
        if (count < 0) return -1;
        int n = process(count, base_type::_in->readBuf, base_type::out.writeBuf);
        base_type::_in->flush();
        if (n < 0 || !base_type::out.swap(count)) return -1;
        return count;
    }

protected:
    void params() {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        gpu::ok(sdrgpu_fast_agc_set(_h.h, _setPoint, _maxGain, _rate, _initGain), "fast_agc_set");
    }
    double _setPoint = 1, _maxGain = 1, _rate = 0, _initGain = 1;
    gpu::Handle _h;
};
}  // namespace dsp::loop
