// GPU-backed dsp::digital::BinarySlicer -- drop-in for core/src/dsp/digital/binary_slicer.h
// (out = in > 0.0f; sdrpp_amd/csrc/symsync.hip). process() is a member here (static in the reference):
// it runs through the block's device handle.
#pragma once
#include "../processor.h"
#include "../sdrgpu_handle.h"

namespace dsp::digital {
class BinarySlicer : public Processor<float, uint8_t> {
    using base_type = Processor<float, uint8_t>;
public:
    BinarySlicer() {}
    BinarySlicer(stream<float>* in) { init(in); }
    void init(stream<float>* in) {
        sdrgpu_block* h = nullptr;
        gpu::ok(sdrgpu_binary_slicer_create(&h, _h.bind(gpu::device())), "binary_slicer_create");
        _h.reset(h);
        base_type::init(in);
    }
    inline int process(int count, const float* in, uint8_t* out) { return _h.process(in, count, out, "binary_slicer"); }
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
}  // namespace dsp::digital
