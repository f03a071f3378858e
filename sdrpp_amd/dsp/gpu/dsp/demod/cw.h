// GPU-backed dsp::demod::CW<T> -- drop-in for core/src/dsp/demod/cw.h (T = float or stereo_t):
// xlate by the tone -> real part -> AGC (cw.h:72-85) on the device. setTone keeps the xlator's phase
// (cw.h:30-35); setSamplerate rebuilds the chain (the AGC gain is carried over).
#pragma once
#include <type_traits>
#include "../processor.h"
#include "../sdrgpu_handle.h"
// the reference header's own includes (core/src/dsp/demod/cw.h): callers such as
// decoder_modules/radio/src/demodulators/*.h rely on them transitively. Headers that exist
// only in the SDR++ tree are guarded, so the block-API mirror build skips them.
#include "../channel/frequency_xlator.h"
#if __has_include("../convert/complex_to_real.h")
#include "../convert/complex_to_real.h"
#endif
#include "../loop/agc.h"
#if __has_include("../convert/mono_to_stereo.h")
#include "../convert/mono_to_stereo.h"
#endif

namespace dsp::demod {
template <class T>
class CW : public Processor<complex_t, T> {
    using base_type = Processor<complex_t, T>;
    static_assert(std::is_same_v<T, float> || std::is_same_v<T, stereo_t>, "CW<T>: T = float or stereo_t");
public:
    CW() {}
    void init(stream<complex_t>* in, double tone, bool agcEnabled, double agcAttack, double agcDecay, double samplerate) {
        _tone = tone; _samplerate = samplerate; _agcEnabled = agcEnabled; _attack = agcAttack; _decay = agcDecay;
        rebuild();
        base_type::init(in);
    }
    void setTone(double tone) { std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx); _tone = tone; gpu::ok(sdrgpu_cw_set_tone(_h.h, tone), "cw_set_tone"); }
    void setAGCEnabled(bool enabled) { std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx); _agcEnabled = enabled; gpu::ok(sdrgpu_demod_agc_set_enabled(_h.h, 0, enabled), "cw_set_agc_enabled"); }
    void setAGCGain(float gain) { std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx); gpu::ok(sdrgpu_demod_agc_set_gain(_h.h, 0, gain), "cw_set_agc_gain"); }
    float getAGCGain() { float g = 0.0f; gpu::ok(sdrgpu_demod_agc_get_gain(_h.h, 0, &g), "cw_get_agc_gain"); return g; }
    void setAGCAttack(double attack) { _attack = attack; ad(); }
    void setAGCDecay(double decay) { _decay = decay; ad(); }
    void setSamplerate(double samplerate) {
        std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx);
        _samplerate = samplerate;
        base_type::tempStop();
        float g = getAGCGain();
        rebuild();
        setAGCGain(g);
        base_type::tempStart();
    }
    int process(int count, const complex_t* in, T* out) { return _h.process(in, count, out, "cw"); }
    int run() override {
        int count = base_type::_in->read();
        if (count < 0) return -1;
        int n = process(count, base_type::_in->readBuf, base_type::out.writeBuf);
        base_type::_in->flush();
        if (n < 0 || !base_type::out.swap(count)) return -1;
        return count;
    }

protected:
    void ad() { std::lock_guard<std::recursive_mutex> lck(base_type::ctrlMtx); gpu::ok(sdrgpu_demod_agc_set_attack_decay(_h.h, _attack, _decay), "cw_set_attack_decay"); }
    void rebuild() {
        sdrgpu_block* h = nullptr;
        gpu::ok(sdrgpu_cw_create(&h, _h.bind(gpu::device()), _tone, _agcEnabled, _attack, _decay, _samplerate,
                                 std::is_same_v<T, stereo_t>), "cw_create");
        _h.reset(h);
    }
    double _tone = 0, _samplerate = 0, _attack = 0, _decay = 0;
    bool _agcEnabled = false;
    gpu::Handle _h;
};
}  // namespace dsp::demod
