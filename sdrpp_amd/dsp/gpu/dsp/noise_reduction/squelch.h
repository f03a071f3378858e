// GPU-backed dsp::noise_reduction::Squelch -- drop-in for core/src/dsp/noise_reduction/squelch.h.
// Per call: level = 20 log10f(mean |x|), the mute state machine of squelch.h:39-53 and the gated
// copy, all on the device (sdrpp_amd/csrc/ifnr.hip). One deliberate deviation: the reference's
// unmute count is a function-local `static int cnt` (squelch.h:40) shared by every squelch of the
// process; here each block has its own.
#pragma once
#include "../processor.h"
#include "../sdrgpu_handle.h"

namespace dsp::noise_reduction {
class Squelch : public Processor<complex_t, complex_t> {
    using base_type = Processor<complex_t, complex_t>;
public:
    Squelch() {}
    Squelch(stream<complex_t>* in, double level) { init(in, level); }
    void init(stream<complex_t>* in, double level) {
        sdrgpu_block* h = nullptr;
        gpu::ok(sdrgpu_squelch_create(&h, _h.bind(gpu::device()), level), "squelch_create");
        _h.reset(h);
        base_type::init(in);
    }
    void setLevel(double level) { std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx); gpu::ok(sdrgpu_squelch_set_level(_h.h, level), "squelch_set_level"); }
    inline int process(int count, const complex_t* in, complex_t* out) { return _h.process(in, count, out, "squelch"); }
    int run() override {
        int count = base_type::_in->read();
        if (count < 0) return -1;
        int n = process(count, base_type::_in->readBuf, base_type::out.writeBuf);
        base_type::_in->flush();
        if (n < 0 || !base_type::out.swap(count)) return -1;
        return count;
    }

protected:
    gpu::Handle _h;
};
}  // namespace dsp::noise_reduction
