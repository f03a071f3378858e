// GPU-backed dsp::noise_reduction::FMIF -- drop-in for core/src/dsp/noise_reduction/fm_if.h (the
// radio module's "IF Noise Reduction"). Per sample: windowed DFT of the last `bins` samples, the
// peak bin kept, sample bins/2 of the back transform out (fm_if.h:45-77), as one GEMM on the f32
// matrix cores (sdrpp_amd/csrc/ifnr.hip). bins in [3, 32]; the history stays on the device.
#pragma once
#include "../processor.h"
#include "../sdrgpu_handle.h"

namespace dsp::noise_reduction {
class FMIF : public Processor<complex_t, complex_t> {
    using base_type = Processor<complex_t, complex_t>;
public:
    FMIF() {}
    FMIF(stream<complex_t>* in, int bins) { init(in, bins); }
    void init(stream<complex_t>* in, int bins) {
        sdrgpu_block* h = nullptr;
        gpu::ok(sdrgpu_fmif_create(&h, _h.bind(gpu::device()), bins), "fmif_create");
        _h.reset(h);
        base_type::init(in);
    }
    void setBins(int bins) {   // new window, history cleared (fm_if.h:26-34)
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        base_type::tempStop();
        gpu::ok(sdrgpu_fmif_set_bins(_h.h, bins), "fmif_set_bins");
        base_type::tempStart();
    }
    void reset() {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        base_type::tempStop();
        gpu::ok(sdrgpu_block_reset(_h.h), "fmif_reset");
        base_type::tempStart();
    }
    int process(int count, const complex_t* in, complex_t* out) { return _h.process(in, count, out, "fmif"); }
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
