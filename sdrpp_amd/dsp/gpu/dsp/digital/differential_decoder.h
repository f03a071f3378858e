// GPU-backed dsp::digital::DifferentialDecoder -- drop-in for core/src/dsp/digital/differential_decoder.h
// (out[i] = (in[i] - in[i-1] + modulus) % modulus, the previous call's last symbol carried on the device;
// sdrpp_amd/csrc/symsync.hip). setModulus / setInitSym rebuild the handle: the carried symbol restarts
// at initSym, as after reset().
#pragma once
#include "../processor.h"
#include "../sdrgpu_handle.h"

namespace dsp::digital {
class DifferentialDecoder : public Processor<uint8_t, uint8_t> {
    using base_type = Processor<uint8_t, uint8_t>;
public:
    DifferentialDecoder() {}
    // (differential_decoder.h:11 leaves the modulus unset; here it is 2 until init / setModulus)
    DifferentialDecoder(stream<uint8_t>* in) { create(); base_type::init(in); }
    void init(stream<uint8_t>* in, uint8_t modulus, uint8_t initSym = 0) {
        _modulus = modulus;
        _initSym = initSym;
        create();
        base_type::init(in);
    }
    void setModulus(uint8_t modulus) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        _modulus = modulus;
        create();
    }
    void setInitSym(uint8_t initSym) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        _initSym = initSym;
        create();
    }
    void reset() {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        base_type::tempStop();
        gpu::ok(sdrgpu_block_reset(_h.h), "differential_decoder_reset");
        base_type::tempStart();
    }
    inline int process(int count, const uint8_t* in, uint8_t* out) { return _h.process(in, count, out, "differential_decoder"); }
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
        gpu::ok(sdrgpu_differential_decoder_create(&h, _h.bind(gpu::device()), _modulus, _initSym), "differential_decoder_create");
        _h.reset(h);
    }
    uint8_t _modulus = 2, _initSym = 0;
    gpu::Handle _h;
};
}  // namespace dsp::digital
