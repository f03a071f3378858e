// GPU-backed dsp::noise_reduction::NoiseBlanker -- drop-in for
// core/src/dsp/noise_reduction/noise_blanker.h. The recurrence runs on the device bit-identically
// to noise_blanker.h:38-57 (sdrpp_amd/csrc/loops.hip); the setters keep the running amplitude.
#pragma once
#include "../processor.h"
#include "../sdrgpu_handle.h"

namespace dsp::noise_reduction {
class NoiseBlanker : public Processor<complex_t, complex_t> {
    using base_type = Processor<complex_t, complex_t>;
public:
    NoiseBlanker() {}
    NoiseBlanker(stream<complex_t>* in, double rate, double level) { init(in, rate, level); }
    void init(stream<complex_t>* in, double rate, double level) {
        _rate = rate; _level = level;
        sdrgpu_block* h = nullptr;
        gpu::ok(sdrgpu_noise_blanker_create(&h, _h.bind(gpu::device()), rate, level), "noise_blanker_create");
        _h.reset(h);
        base_type::init(in);
    }
    void setRate(double rate) { _rate = rate; params(); }
    void setLevel(double level) { _level = level; params(); }
    void reset() { std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx); gpu::ok(sdrgpu_block_reset(_h.h), "noise_blanker_reset"); }
    inline int process(int count, complex_t* in, complex_t* out) { return _h.process(in, count, out, "noise_blanker"); }
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
        gpu::ok(sdrgpu_noise_blanker_set(_h.h, _rate, _level), "noise_blanker_set");
    }
    double _rate = 0, _level = 0;
    gpu::Handle _h;
};
}  // namespace dsp::noise_reduction
