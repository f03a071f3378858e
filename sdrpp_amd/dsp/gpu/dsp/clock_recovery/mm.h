// GPU-backed dsp::clock_recovery::MM<T> -- drop-in for core/src/dsp/clock_recovery/mm.h (T = float or
// complex_t). The loop runs on the device (sdrpp_amd/csrc/symsync.hip): output count and outputs are
// those of mm.h:100-156 with the interpolator dot product in ascending tap order (VOLK's generic
// kernel) and a history that starts as zeros (include/sdrgpu.h lists the deviations). Parameters with
// omega * (1 - omegaRelLimit) - muGain < 1 are refused (reported, the previous ones stay).
#pragma once
#include <type_traits>
#include "../processor.h"
#include "../sdrgpu_handle.h"

namespace dsp::clock_recovery {
template <class T>
class MM : public Processor<T, T> {
    using base_type = Processor<T, T>;
    static_assert(std::is_same_v<T, float> || std::is_same_v<T, complex_t>, "MM<T>: T = float or complex_t");
public:
    MM() {}
    MM(stream<T>* in, double omega, double omegaGain, double muGain, double omegaRelLimit, int interpPhaseCount = 128, int interpTapCount = 8) {
        init(in, omega, omegaGain, muGain, omegaRelLimit, interpPhaseCount, interpTapCount);
    }
    void init(stream<T>* in, double omega, double omegaGain, double muGain, double omegaRelLimit, int interpPhaseCount = 128, int interpTapCount = 8) {
        _omega = omega; _omegaGain = omegaGain; _muGain = muGain; _omegaRelLimit = omegaRelLimit;
        _interpPhaseCount = interpPhaseCount; _interpTapCount = interpTapCount;
        create();
        base_type::init(in);
    }
    void setOmega(double omega) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        base_type::tempStop();
        if (gpu::ok(sdrgpu_mm_set_omega(_h.h, omega), "mm_set_omega")) _omega = omega;
        base_type::tempStart();
    }
    void setOmegaGain(double omegaGain) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        if (gpu::ok(sdrgpu_mm_set_gains(_h.h, omegaGain, _muGain), "mm_set_gains")) _omegaGain = omegaGain;
    }
    void setMuGain(double muGain) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        if (gpu::ok(sdrgpu_mm_set_gains(_h.h, _omegaGain, muGain), "mm_set_gains")) _muGain = muGain;
    }
    void setOmegaRelLimit(double omegaRelLimit) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        if (gpu::ok(sdrgpu_mm_set_omega_rel_limit(_h.h, omegaRelLimit), "mm_set_omega_rel_limit")) _omegaRelLimit = omegaRelLimit;
    }
    // a new bank and a new work buffer (mm.h:73-85); here the loop state restarts with them
    void setInterpParams(int interpPhaseCount, int interpTapCount) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        base_type::tempStop();
        _interpPhaseCount = interpPhaseCount; _interpTapCount = interpTapCount;
        create();
        base_type::tempStart();
    }
    void reset() {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        base_type::tempStop();
        gpu::ok(sdrgpu_block_reset(_h.h), "mm_reset");
        base_type::tempStart();
    }
    inline int process(int count, const T* in, T* out) { return _h.process(in, count, out, "mm"); }
    int run() override {
        int count = base_type::_in->read();
        if (count < 0) return -1;
        int outCount = process(count, base_type::_in->readBuf, base_type::out.writeBuf);
        base_type::_in->flush();
        if (outCount < 0) return -1;
        if (outCount) {   // swap if some data was generated (mm.h:164-168)
            if (!base_type::out.swap(outCount)) return -1;
        }
        return outCount;
    }

protected:
    void create() {
        sdrgpu_block* h = nullptr;
        gpu::ok(sdrgpu_mm_create(&h, _h.bind(gpu::device()), std::is_same_v<T, complex_t> ? SDRGPU_C64 : SDRGPU_F32, _omega, _omegaGain,
                                 _muGain, _omegaRelLimit, _interpPhaseCount, _interpTapCount), "mm_create");
        _h.reset(h);
    }
    double _omega = 0, _omegaGain = 0, _muGain = 0, _omegaRelLimit = 0;
    int _interpPhaseCount = 128, _interpTapCount = 8;
    gpu::Handle _h;
};
}  // namespace dsp::clock_recovery
