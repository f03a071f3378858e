// Second reference probe (test infrastructure; built only where the reference tree exists, output in
// oracle/_ref/). Includes the reference's OWN stateful block headers -- loops, symbol recovery, IF
// noise reduction and the PSK / GFSK chains -- from where the reference lies and calls their
// process() directly, so the numpy restatements in tests/_restated.py, the C oracle's loops and the
// device kernels are pinned against reference code, not against a reading of it. VOLK, FFTW and the
// host runtime are replaced by oracle/ref_standins.cpp. No thread is ever started.
//
//   ref_blocks <mode> <calls> [parameters...]
//
// <calls> is a comma list run in order: a number is one process() call of that many input samples
// (0 included); `r` calls reset() (MM and the channel-chain modes), `o<omega>` setOmega() and `i<P>x<T>`
// setInterpParams() (MM); for the channel-chain modes `w<rad>` is the xlator's setOffset(), `f<hz>`
// RxVFO::setOffset(), `d<n>` setDecimation(), `t<k>` setTaps() to the k-th tap set and `v<rad>`
// setDeviation(). Input samples are raw on stdin (as many as the calls sum to); the modes that take
// tap sets (fir_*, poly_*, ddc, ddcfm) read them first: int32 number of sets, then per set int32 count
// and the taps, raw. They stay allocated for the whole run (tap<T> is not owned by the block). stdout:
// int32 number of process() calls, int32 output count of each, then every call's outputs, raw, in
// order. The rds mode appends every call's bits (uint8) after the soft symbols, the ddcfm mode every
// call's FIR-stage outputs (complex_t).
//
//   fastagc_f|fastagc_c  setPoint maxGain rate initGain     loop::FastAGC<float|complex_t>
//   costas  order bandwidth [initPhase initFreq minFreq maxFreq]
//                                                           loop::Costas<2|4|8>, init() as wfm.h calls it
//   mm_f|mm_c  omega omegaGain muGain omegaRelLimit         clock_recovery::MM<float|complex_t> (128, 8)
//   slicer                                                  digital::BinarySlicer
//   diff  modulus initSym                                   digital::DifferentialDecoder
//   nb  rate level                                          noise_reduction::NoiseBlanker
//   squelch  level                                          noise_reduction::Squelch, one object
//   fmif  bins                                              noise_reduction::FMIF
//   agc_f|agc_c  setPoint attack decay maxGain maxOutputAmp initGain   loop::AGC<float|complex_t>
//   dcb_f|dcb_c  rate                                       correction::DCBlocker<float|complex_t>
//   deemp_f|deemp_s  tau samplerate                         filter::Deemphasis<float|stereo_t>
//   psk  order symbolrate samplerate rrcTaps rrcBeta agcRate costasBw omegaGain muGain omegaRelLimit
//   gfsk  symbolrate samplerate deviation rrcTaps rrcBeta omegaGain muGain omegaRelLimit
//   rds                                                     the blocks and calls of the radio module's wfm.h:57-68
// Channel chain:
//   xlator  w                                               channel::FrequencyXlator
//   fir_ff|fir_cf|fir_cc  D                                 filter::DecimatingFIR<D, T> for D > 1, filter::FIR<D, T> for D = 1
//   pdec_f|pdec_c  ratio                                    multirate::PowerDecimator<float|complex_t>
//   poly_f|poly_c  interp decim                             multirate::PolyphaseResampler<float|complex_t>
//   rres_f|rres_c  in out                                   multirate::RationalResampler<float|complex_t>
//   rxvfo  in out bw offset                                 channel::RxVFO
//   quad  dev                                               demod::Quadrature
//   fm  samplerate bandwidth lowPass highPass               demod::FM<float>
//   ddc  w D                                                FrequencyXlator -> DecimatingFIR<complex_t, float>, block by block
//   ddcfm  w D dev                                          the same -> Quadrature
// Analogue demodulators. Ops: `r` reset() (AM, BroadcastFM), `g<x>` setAGCGain(), `e<0|1>` setAGCEnabled() (SSB, CW),
// `a<att>x<dec>` setAGCAttack() + setAGCDecay(), `b<rate>` AM::setDCBlockRate(), `w<hz>` CW::setTone(), `R<0|1>`
// BroadcastFM::setRDSOut(). The _s modes write stereo_t. After the outputs the am modes append the low-pass filter's
// input of every call (float; taken from a twin block given the same calls whose low-pass is one unit tap), the bfm
// mode the RDS output count of every call (int32) and then every call's RDS samples (complex_t).
//   am_f|am_s  agcMode bandwidth attack decay dcBlockRate samplerate     demod::AM<float|stereo_t>
//   ssb_f|ssb_s  mode bandwidth samplerate agcEnabled attack decay       demod::SSB<float|stereo_t>
//   cw_f|cw_s  tone agcEnabled attack decay samplerate                   demod::CW<float|stereo_t>
//   bfm  deviation samplerate stereo lowPass rdsOut                      demod::BroadcastFM
// Carrier loops and the Meteor demodulator (the decoder module's header, on the include path). Ops: `r` reset() (all
// four), `b<0|1>` setBrokenModulation() (mcostas, meteor: the letter's meaning is per mode, as `w`'s is),
// `q<0|1>` Meteor::setOQPSK().
//   pll|cpll  bandwidth initPhase initFreq minFreq maxFreq               loop::PLL | loop::CarrierTrackingPLL
//   mcostas  bandwidth broken initPhase initFreq minFreq maxFreq         loop::MeteorCostas
//   meteor  symbolrate samplerate rrcTaps rrcBeta agcRate costasBw broken oqpsk omegaGain muGain omegaRelLimit
//                                                                        demod::Meteor
// Design code (no stdin, <calls> ignored; stdout float32 only):
//   rrc  count beta Ts                                      taps::rootRaisedCosine<float>
//   mmbank  P T                                             the bank MM builds for itself, [P][T]
//   fmifwin  bins                                           the window FMIF builds for itself
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>
#include <dsp/types.h>
#include <dsp/loop/fast_agc.h>
#include <dsp/loop/costas.h>
#include <dsp/loop/agc.h>
#include <dsp/clock_recovery/mm.h>
#include <dsp/digital/binary_slicer.h>
#include <dsp/digital/differential_decoder.h>
#include <dsp/noise_reduction/noise_blanker.h>
#include <dsp/noise_reduction/squelch.h>
#include <dsp/noise_reduction/fm_if.h>
#include <dsp/correction/dc_blocker.h>
#include <dsp/filter/deephasis.h>
#include <dsp/filter/fir.h>
#include <dsp/taps/root_raised_cosine.h>
#include <dsp/taps/band_pass.h>
#include <dsp/convert/complex_to_real.h>
#include <dsp/math/hz_to_rads.h>
#include <dsp/demod/psk.h>
#include <dsp/demod/gfsk.h>
#include <dsp/channel/rx_vfo.h>
#include <dsp/filter/decimating_fir.h>
#include <dsp/multirate/power_decimator.h>
#include <dsp/multirate/polyphase_resampler.h>
#include <dsp/multirate/rational_resampler.h>
#include <dsp/demod/quadrature.h>
#include <dsp/demod/fm.h>
#include <dsp/demod/am.h>
#include <dsp/demod/ssb.h>
#include <dsp/demod/cw.h>
#include <dsp/demod/broadcast_fm.h>
#include <dsp/loop/pll.h>
#include <dsp/loop/carrier_tracking_pll.h>
#include "meteor_demod.h"

using dsp::complex_t;
using dsp::stereo_t;

struct Op {
    char kind;      // 'p' process, 'r' reset, 'o' setOmega, 'i' setInterpParams, 'w' 'f' 'd' 't' 'v' the chain's setters,
                    // 'g' 'e' 'a' 'b' 'R' 'q' the demodulators'
    int count = 0, a = 0, b = 0;
    double v = 0.0, v2 = 0.0;
};

static std::vector<Op> parseCalls(const char* s) {
    std::vector<Op> ops;
    std::string str(s), tok;
    size_t pos = 0;
    while (pos <= str.size()) {
        size_t e = str.find(',', pos);
        if (e == std::string::npos) { e = str.size(); }
        tok = str.substr(pos, e - pos);
        pos = e + 1;
        if (tok.empty()) { continue; }
        Op op;
        if (tok[0] == 'r') { op.kind = 'r'; }
        else if (tok[0] == 'o') { op.kind = 'o'; op.v = strtod(tok.c_str() + 1, NULL); }
        else if (tok[0] == 'i') { op.kind = 'i'; sscanf(tok.c_str() + 1, "%dx%d", &op.a, &op.b); }
        else if (tok[0] == 'w' || tok[0] == 'f' || tok[0] == 'v') { op.kind = tok[0]; op.v = strtod(tok.c_str() + 1, NULL); }
        else if (tok[0] == 'g' || tok[0] == 'b') { op.kind = tok[0]; op.v = strtod(tok.c_str() + 1, NULL); }
        else if (tok[0] == 'a') { op.kind = 'a'; sscanf(tok.c_str() + 1, "%lfx%lf", &op.v, &op.v2); }
        else if (tok[0] == 'e' || tok[0] == 'R' || tok[0] == 'q') { op.kind = tok[0]; op.a = atoi(tok.c_str() + 1); }
        else if (tok[0] == 'd' || tok[0] == 't') { op.kind = tok[0]; op.a = atoi(tok.c_str() + 1); }
        else { op.kind = 'p'; op.count = atoi(tok.c_str()); }
        ops.push_back(op);
    }
    return ops;
}

template <class T>
static std::vector<T> readInput(size_t n) {
    std::vector<T> x(n + 1);
    if (fread(x.data(), sizeof(T), n, stdin) != n) { fprintf(stderr, "ref_blocks: short input\n"); exit(3); }
    return x;
}

static size_t outPerIn = 1;          // output capacity per input sample (the interpolating resamplers: more than 1)
static std::vector<uint8_t> tail;    // written after everything else (ddcfm: the FIR-stage outputs)
static std::vector<uint8_t> tail2;   // written after `tail` (bfm: the RDS samples, after their counts)

// Runs the process() calls of `ops` over stdin; `other` handles the remaining kinds.
template <class I, class O>
static int runCalls(const std::vector<Op>& ops, std::function<int(int, I*, O*)> proc,
                    std::function<void(const Op&)> other = nullptr,
                    std::vector<uint8_t>* second = nullptr, std::function<void(int, uint8_t*)> fillSecond = nullptr) {
    size_t total = 0;
    for (auto& op : ops) { total += op.kind == 'p' ? op.count : 0; }
    std::vector<I> x = readInput<I>(total);
    std::vector<O> y((total + ops.size()) * outPerIn + 1);
    std::vector<int32_t> counts;
    size_t ip = 0, op_ = 0;
    for (auto& op : ops) {
        if (op.kind != 'p') {
            if (!other) { fprintf(stderr, "ref_blocks: this mode takes process() calls only\n"); return 2; }
            other(op);
            continue;
        }
        int n = proc(op.count, x.data() + ip, y.data() + op_);
        if (second) {
            size_t at = second->size();
            second->resize(at + n);
            fillSecond(n, second->data() + at);
        }
        counts.push_back(n);
        ip += op.count;
        op_ += n;
    }
    int32_t nc = (int32_t)counts.size();
    fwrite(&nc, sizeof(nc), 1, stdout);
    fwrite(counts.data(), sizeof(int32_t), counts.size(), stdout);
    fwrite(y.data(), sizeof(O), op_, stdout);
    if (second) { fwrite(second->data(), 1, second->size(), stdout); }
    fwrite(tail.data(), 1, tail.size(), stdout);
    fwrite(tail2.data(), 1, tail2.size(), stdout);
    return 0;
}

// A block in zero-filled storage, as an object of static storage duration would be: some members have
// no initialiser and are not set by init() (Quadrature's previous sample, demod/quadrature.h:84), so a
// block on the stack would start from whatever the stack held. Never destroyed: the process ends.
template <class T>
static T& zeroed() {
    return *new (calloc(1, sizeof(T))) T();
}

template <class T>
struct OpenMM : dsp::clock_recovery::MM<T> {
    dsp::multirate::PolyphaseBank<float>& bank() { return this->interpBank; }
};

struct OpenFMIF : dsp::noise_reduction::FMIF {
    float* win() { return fftWin; }
};

template <class T>
static int runFastAGC(const std::vector<Op>& ops, char** p) {
    dsp::loop::FastAGC<T>& b = zeroed<dsp::loop::FastAGC<T>>();
    b.init(NULL, atof(p[0]), atof(p[1]), atof(p[2]), atof(p[3]));
    return runCalls<T, T>(ops, [&](int n, T* in, T* out) { return b.process(n, in, out); });
}

template <int ORDER>
static int runCostas(const std::vector<Op>& ops, int np, char** p) {
    dsp::loop::Costas<ORDER>& b = zeroed<dsp::loop::Costas<ORDER>>();
    if (np == 1) { b.init(NULL, atof(p[0])); }
    else { b.init(NULL, atof(p[0]), atof(p[1]), atof(p[2]), atof(p[3]), atof(p[4])); }
    return runCalls<complex_t, complex_t>(ops, [&](int n, complex_t* in, complex_t* out) { return b.process(n, in, out); });
}

template <class T>
static int runMM(const std::vector<Op>& ops, char** p) {
    dsp::clock_recovery::MM<T>& b = zeroed<dsp::clock_recovery::MM<T>>();
    b.init(NULL, atof(p[0]), atof(p[1]), atof(p[2]), atof(p[3]));
    return runCalls<T, T>(ops, [&](int n, T* in, T* out) { return b.process(n, in, out); }, [&](const Op& op) {
        if (op.kind == 'r') { b.reset(); }
        if (op.kind == 'o') { b.setOmega(op.v); }
        if (op.kind == 'i') { b.setInterpParams(op.a, op.b); }
    });
}

template <class T>
static int runAGC(const std::vector<Op>& ops, char** p) {
    dsp::loop::AGC<T>& b = zeroed<dsp::loop::AGC<T>>();
    b.init(NULL, atof(p[0]), atof(p[1]), atof(p[2]), atof(p[3]), atof(p[4]), atof(p[5]));
    return runCalls<T, T>(ops, [&](int n, T* in, T* out) { return b.process(n, in, out); });
}

template <class T>
static int runDCB(const std::vector<Op>& ops, char** p) {
    dsp::correction::DCBlocker<T>& b = zeroed<dsp::correction::DCBlocker<T>>();
    b.init(NULL, atof(p[0]));
    return runCalls<T, T>(ops, [&](int n, T* in, T* out) { return b.process(n, in, out); });
}

template <class T>
static int runDeemp(const std::vector<Op>& ops, char** p) {
    dsp::filter::Deemphasis<T>& b = zeroed<dsp::filter::Deemphasis<T>>();
    b.init(NULL, atof(p[0]), atof(p[1]));
    // (an empty call is not passed on: filter/deephasis.h:58-72 writes out[0] and reads out[count - 1])
    return runCalls<T, T>(ops, [&](int n, T* in, T* out) { return n ? b.process(n, in, out) : 0; });
}

template <int ORDER>
static int runPSK(const std::vector<Op>& ops, char** p) {
    dsp::demod::PSK<ORDER>& b = zeroed<dsp::demod::PSK<ORDER>>();
    b.init(NULL, atof(p[0]), atof(p[1]), atoi(p[2]), atof(p[3]), atof(p[4]), atof(p[5]), atof(p[6]), atof(p[7]), atof(p[8]));
    return runCalls<complex_t, complex_t>(ops, [&](int n, complex_t* in, complex_t* out) { return b.process(n, in, out); });
}

static int runRDS(const std::vector<Op>& ops) {
    // the members and init calls of the radio module's WFM demodulator; the stream pointers are
    // NULL because process() is called directly, block by block, in the order the streams connect
    dsp::loop::FastAGC<complex_t>& agc = zeroed<dsp::loop::FastAGC<complex_t>>();
    dsp::loop::Costas<2>& costas = zeroed<dsp::loop::Costas<2>>();
    dsp::loop::Costas<2>& costas2 = zeroed<dsp::loop::Costas<2>>();
    dsp::tap<complex_t> taps;
    dsp::filter::FIR<complex_t, complex_t>& fir = zeroed<dsp::filter::FIR<complex_t, complex_t>>();
    dsp::clock_recovery::MM<float>& recov = zeroed<dsp::clock_recovery::MM<float>>();
    dsp::digital::DifferentialDecoder& diff = zeroed<dsp::digital::DifferentialDecoder>();
    agc.init(NULL, 1.0, 1e6, 0.1);
    costas.init(NULL, 0.005f);
    taps = dsp::taps::bandPass<complex_t>(0, 2375, 100, 5000);
    fir.init(NULL, taps);
    double baudfreq = dsp::math::hzToRads(2375.0 / 2.0, 5000);
    costas2.init(NULL, 0.01, 0.0, baudfreq, baudfreq - (baudfreq * 0.1), baudfreq + (baudfreq * 0.1));
    recov.init(NULL, 5000.0 / (2375.0 / 2.0), 1e-6, 0.01, 0.01);
    diff.init(NULL, 2);
    size_t cap = 1;
    for (auto& op : ops) { cap = std::max<size_t>(cap, op.count + 1); }
    std::vector<complex_t> a(cap), b(cap);
    std::vector<float> f(cap);
    std::vector<uint8_t> s(cap), bits;
    float* soft = NULL;
    return runCalls<complex_t, float>(ops, [&](int n, complex_t* in, float* out) {
        agc.process(n, in, a.data());
        costas.process(n, a.data(), b.data());
        fir.process(n, b.data(), a.data());
        costas2.process(n, a.data(), b.data());
        dsp::convert::ComplexToReal::process(n, b.data(), f.data());
        soft = out;
        return recov.process(n, f.data(), out);
    }, nullptr, &bits, [&](int m, uint8_t* out) {
        dsp::digital::BinarySlicer::process(m, soft, s.data());
        diff.process(m, s.data(), out);
    });
}

// ------------------------------------------------------------------ channel chain
template <class T>
static std::vector<dsp::tap<T>> readTapSets() {
    int32_t ns = 0, n = 0;
    if (fread(&ns, sizeof(ns), 1, stdin) != 1 || ns < 1) { fprintf(stderr, "ref_blocks: no tap sets\n"); exit(3); }
    std::vector<dsp::tap<T>> sets(ns);
    for (auto& t : sets) {
        if (fread(&n, sizeof(n), 1, stdin) != 1 || n < 1) { fprintf(stderr, "ref_blocks: bad tap set\n"); exit(3); }
        t = dsp::taps::alloc<T>(n);
        if (fread(t.taps, sizeof(T), n, stdin) != (size_t)n) { fprintf(stderr, "ref_blocks: short tap set\n"); exit(3); }
    }
    return sets;
}

static void badOp(const Op& op) {
    fprintf(stderr, "ref_blocks: this mode has no op '%c'\n", op.kind);
    exit(2);
}

template <class T>
static dsp::tap<T>& tapSet(std::vector<dsp::tap<T>>& sets, const Op& op) {
    if (op.a < 0 || op.a >= (int)sets.size()) { fprintf(stderr, "ref_blocks: no tap set %d\n", op.a); exit(2); }
    return sets[op.a];
}

template <class D, class T>
static int runFIR(const std::vector<Op>& ops, int decim) {
    static std::vector<dsp::tap<T>> sets = readTapSets<T>();
    if (decim > 1) {
        auto& b = zeroed<dsp::filter::DecimatingFIR<D, T>>();
        b.init(NULL, sets[0], decim);
        return runCalls<D, D>(ops, [&](int n, D* in, D* out) { return b.process(n, in, out); }, [&](const Op& op) {
            if (op.kind == 'r') { b.reset(); }
            else if (op.kind == 't') { b.setTaps(tapSet(sets, op)); }
            else if (op.kind == 'd') { b.setDecimation(op.a); }
            else { badOp(op); }
        });
    }
    auto& b = zeroed<dsp::filter::FIR<D, T>>();
    b.init(NULL, sets[0]);
    return runCalls<D, D>(ops, [&](int n, D* in, D* out) { return b.process(n, in, out); }, [&](const Op& op) {
        if (op.kind == 'r') { b.reset(); }
        else if (op.kind == 't') { b.setTaps(tapSet(sets, op)); }
        else { badOp(op); }
    });
}

template <class T>
static int runPdec(const std::vector<Op>& ops, char** p) {
    auto& b = zeroed<dsp::multirate::PowerDecimator<T>>();
    b.init(NULL, atoi(p[0]));
    return runCalls<T, T>(ops, [&](int n, T* in, T* out) { return b.process(n, in, out); },
                          [&](const Op& op) { if (op.kind == 'r') { b.reset(); } else { badOp(op); } });
}

template <class T>
static int runPoly(const std::vector<Op>& ops, char** p) {
    static std::vector<dsp::tap<float>> sets = readTapSets<float>();
    auto& b = zeroed<dsp::multirate::PolyphaseResampler<T>>();
    b.init(NULL, atoi(p[0]), atoi(p[1]), sets[0]);
    outPerIn = atoi(p[0]) / atoi(p[1]) + 1;
    return runCalls<T, T>(ops, [&](int n, T* in, T* out) { return b.process(n, in, out); },
                          [&](const Op& op) { if (op.kind == 'r') { b.reset(); } else { badOp(op); } });
}

template <class T>
static int runRres(const std::vector<Op>& ops, char** p) {
    auto& b = zeroed<dsp::multirate::RationalResampler<T>>();
    b.init(NULL, atof(p[0]), atof(p[1]));
    outPerIn = (size_t)(atof(p[1]) / atof(p[0])) + 1;
    return runCalls<T, T>(ops, [&](int n, T* in, T* out) { return b.process(n, in, out); },
                          [&](const Op& op) { if (op.kind == 'r') { b.reset(); } else { badOp(op); } });
}

static int runRxVFO(const std::vector<Op>& ops, char** p) {
    auto& b = zeroed<dsp::channel::RxVFO>();
    b.init(NULL, atof(p[0]), atof(p[1]), atof(p[2]), atof(p[3]));
    outPerIn = (size_t)(atof(p[1]) / atof(p[0])) + 1;
    return runCalls<complex_t, complex_t>(ops, [&](int n, complex_t* in, complex_t* out) { return b.process(n, in, out); },
                                          [&](const Op& op) {
        if (op.kind == 'r') { b.reset(); }
        else if (op.kind == 'f') { b.setOffset(op.v); }
        else { badOp(op); }
    });
}

// xlator -> DecimatingFIR<complex_t, float> [-> Quadrature], each block's process() called in the order
// the streams would connect them; reset() resets every block of the chain
static int runDDC(const std::vector<Op>& ops, char** p, bool fm) {
    static std::vector<dsp::tap<float>> sets = readTapSets<float>();
    auto& x = zeroed<dsp::channel::FrequencyXlator>();
    auto& f = zeroed<dsp::filter::DecimatingFIR<complex_t, float>>();
    auto& q = zeroed<dsp::demod::Quadrature>();
    x.init(NULL, atof(p[0]));
    f.init(NULL, sets[0], atoi(p[1]));
    if (fm) { q.init(NULL, atof(p[2])); }
    size_t cap = 1;
    for (auto& op : ops) { cap = std::max<size_t>(cap, op.count + 1); }
    std::vector<complex_t> a(cap), z(cap);
    auto other = [&](const Op& op) {
        if (op.kind == 'r') { x.reset(); f.reset(); if (fm) { q.reset(); } }
        else if (op.kind == 't') { f.setTaps(tapSet(sets, op)); }
        else if (op.kind == 'd') { f.setDecimation(op.a); }
        else if (op.kind == 'v' && fm) { q.setDeviation(op.v); }
        else { badOp(op); }
    };
    if (!fm) {
        return runCalls<complex_t, complex_t>(ops, [&](int n, complex_t* in, complex_t* out) {
            x.process(n, in, a.data());
            return f.process(n, a.data(), out);
        }, other);
    }
    return runCalls<complex_t, float>(ops, [&](int n, complex_t* in, float* out) {
        x.process(n, in, a.data());
        int m = f.process(n, a.data(), z.data());
        const uint8_t* raw = (const uint8_t*)z.data();
        tail.insert(tail.end(), raw, raw + m * sizeof(complex_t));
        return q.process(m, z.data(), out);
    }, other);
}

// ------------------------------------------------------------------ analogue demodulators
template <class V>
static void append(std::vector<uint8_t>& to, const V* v, size_t n) {
    const uint8_t* raw = (const uint8_t*)v;
    to.insert(to.end(), raw, raw + n * sizeof(V));
}

// AM with its low-pass replaced by one unit tap: its output is the low-pass filter's input
template <class T>
struct UnitLowPassAM : dsp::demod::AM<T> {
    dsp::tap<float> unit;
    void unitLowPass() {
        unit = dsp::taps::alloc<float>(1);
        unit.taps[0] = 1.0f;
        this->lpf.setTaps(unit);
    }
};

template <class T>
static int runAM(const std::vector<Op>& ops, char** p) {
    typedef typename dsp::demod::AM<T>::AGCMode Mode;
    auto& b = zeroed<dsp::demod::AM<T>>();
    auto& twin = zeroed<UnitLowPassAM<T>>();
    b.init(NULL, (Mode)atoi(p[0]), atof(p[1]), atof(p[2]), atof(p[3]), atof(p[4]), atof(p[5]));
    twin.init(NULL, (Mode)atoi(p[0]), atof(p[1]), atof(p[2]), atof(p[3]), atof(p[4]), atof(p[5]));
    twin.unitLowPass();
    size_t cap = 1;
    for (auto& op : ops) { cap = std::max<size_t>(cap, op.count + 1); }
    std::vector<T> z(cap);
    return runCalls<complex_t, T>(ops, [&](int n, complex_t* in, T* out) {
        twin.process(n, in, z.data());
        for (int i = 0; i < n; i++) { append(tail, (const float*)&z[i], 1); }   // (stereo_t: l, which equals r)
        return b.process(n, in, out);
    }, [&](const Op& op) {
        if (op.kind == 'r') { b.reset(); twin.reset(); }
        else if (op.kind == 'g') { b.setAGCGain(op.v); twin.setAGCGain(op.v); }
        else if (op.kind == 'a') { b.setAGCAttack(op.v); b.setAGCDecay(op.v2); twin.setAGCAttack(op.v); twin.setAGCDecay(op.v2); }
        else if (op.kind == 'b') { b.setDCBlockRate(op.v); twin.setDCBlockRate(op.v); }
        else { badOp(op); }
    });
}

template <class T>
static int runSSB(const std::vector<Op>& ops, char** p) {
    typedef typename dsp::demod::SSB<T>::Mode Mode;
    auto& b = zeroed<dsp::demod::SSB<T>>();
    b.init(NULL, (Mode)atoi(p[0]), atof(p[1]), atof(p[2]), atoi(p[3]) != 0, atof(p[4]), atof(p[5]));
    return runCalls<complex_t, T>(ops, [&](int n, complex_t* in, T* out) { return b.process(n, in, out); }, [&](const Op& op) {
        if (op.kind == 'e') { b.setAGCEnabled(op.a != 0); }
        else if (op.kind == 'g') { b.setAGCGain(op.v); }
        else if (op.kind == 'a') { b.setAGCAttack(op.v); b.setAGCDecay(op.v2); }
        else { badOp(op); }
    });
}

template <class T>
static int runCW(const std::vector<Op>& ops, char** p) {
    auto& b = zeroed<dsp::demod::CW<T>>();
    b.init(NULL, atof(p[0]), atoi(p[1]) != 0, atof(p[2]), atof(p[3]), atof(p[4]));
    return runCalls<complex_t, T>(ops, [&](int n, complex_t* in, T* out) { return b.process(n, in, out); }, [&](const Op& op) {
        if (op.kind == 'w') { b.setTone(op.v); }
        else if (op.kind == 'e') { b.setAGCEnabled(op.a != 0); }
        else if (op.kind == 'g') { b.setAGCGain(op.v); }
        else if (op.kind == 'a') { b.setAGCAttack(op.v); b.setAGCDecay(op.v2); }
        else { badOp(op); }
    });
}

static int runBFM(const std::vector<Op>& ops, char** p) {
    auto& b = zeroed<dsp::demod::BroadcastFM>();
    b.init(NULL, atof(p[0]), atof(p[1]), atoi(p[2]) != 0, atoi(p[3]) != 0, atoi(p[4]) != 0);
    size_t cap = 1;
    for (auto& op : ops) { cap = std::max<size_t>(cap, op.count + 1); }
    std::vector<complex_t> rds(cap);
    return runCalls<complex_t, stereo_t>(ops, [&](int n, complex_t* in, stereo_t* out) {
        int nrds = 0;
        int m = b.process(n, in, out, nrds, rds.data());
        int32_t c = nrds;
        append(tail, &c, 1);
        append(tail2, rds.data(), nrds);
        return m;
    }, [&](const Op& op) {
        if (op.kind == 'r') { b.reset(); }
        else if (op.kind == 'R') { b.setRDSOut(op.a != 0); }
        else { badOp(op); }
    });
}

// ------------------------------------------------------------------ carrier loops, Meteor
template <class B>
static int runPLL(const std::vector<Op>& ops, char** p) {
    auto& b = zeroed<B>();
    b.init(NULL, atof(p[0]), atof(p[1]), atof(p[2]), atof(p[3]), atof(p[4]));
    return runCalls<complex_t, complex_t>(ops, [&](int n, complex_t* in, complex_t* out) { return b.process(n, in, out); },
                                          [&](const Op& op) { if (op.kind == 'r') { b.reset(); } else { badOp(op); } });
}

int main(int argc, char** argv) {
    if (argc < 3) { return 2; }
    std::string mode = argv[1];
    std::vector<Op> ops = parseCalls(argv[2]);
    char** p = argv + 3;
    int np = argc - 3;

    if (mode == "fastagc_f" && np == 4) { return runFastAGC<float>(ops, p); }
    if (mode == "fastagc_c" && np == 4) { return runFastAGC<complex_t>(ops, p); }
    if (mode == "costas" && (np == 2 || np == 6)) {
        int order = atoi(p[0]);
        if (order == 2) { return runCostas<2>(ops, np - 1, p + 1); }
        if (order == 4) { return runCostas<4>(ops, np - 1, p + 1); }
        if (order == 8) { return runCostas<8>(ops, np - 1, p + 1); }
        return 2;
    }
    if (mode == "mm_f" && np == 4) { return runMM<float>(ops, p); }
    if (mode == "mm_c" && np == 4) { return runMM<complex_t>(ops, p); }
    if (mode == "slicer" && np == 0) {
        return runCalls<float, uint8_t>(ops, [&](int n, float* in, uint8_t* out) { return dsp::digital::BinarySlicer::process(n, in, out); });
    }
    if (mode == "diff" && np == 2) {
        dsp::digital::DifferentialDecoder& b = zeroed<dsp::digital::DifferentialDecoder>();
        b.init(NULL, atoi(p[0]), atoi(p[1]));
        return runCalls<uint8_t, uint8_t>(ops, [&](int n, uint8_t* in, uint8_t* out) { return b.process(n, in, out); });
    }
    if (mode == "nb" && np == 2) {
        dsp::noise_reduction::NoiseBlanker& b = zeroed<dsp::noise_reduction::NoiseBlanker>();
        b.init(NULL, atof(p[0]), atof(p[1]));
        return runCalls<complex_t, complex_t>(ops, [&](int n, complex_t* in, complex_t* out) { return b.process(n, in, out); });
    }
    if (mode == "squelch" && np == 1) {
        dsp::noise_reduction::Squelch& b = zeroed<dsp::noise_reduction::Squelch>();
        b.init(NULL, atof(p[0]));
        return runCalls<complex_t, complex_t>(ops, [&](int n, complex_t* in, complex_t* out) { return b.process(n, in, out); });
    }
    if (mode == "fmif" && np == 1) {
        dsp::noise_reduction::FMIF& b = zeroed<dsp::noise_reduction::FMIF>();
        b.init(NULL, atoi(p[0]));
        return runCalls<complex_t, complex_t>(ops, [&](int n, complex_t* in, complex_t* out) { return b.process(n, in, out); });
    }
    if (mode == "agc_f" && np == 6) { return runAGC<float>(ops, p); }
    if (mode == "agc_c" && np == 6) { return runAGC<complex_t>(ops, p); }
    if (mode == "dcb_f" && np == 1) { return runDCB<float>(ops, p); }
    if (mode == "dcb_c" && np == 1) { return runDCB<complex_t>(ops, p); }
    if (mode == "deemp_f" && np == 2) { return runDeemp<float>(ops, p); }
    if (mode == "deemp_s" && np == 2) { return runDeemp<stereo_t>(ops, p); }
    if (mode == "psk" && np == 10) {
        int order = atoi(p[0]);
        if (order == 2) { return runPSK<2>(ops, p + 1); }
        if (order == 4) { return runPSK<4>(ops, p + 1); }
        return 2;
    }
    if (mode == "gfsk" && np == 8) {
        dsp::demod::GFSK& b = zeroed<dsp::demod::GFSK>();
        b.init(NULL, atof(p[0]), atof(p[1]), atof(p[2]), atoi(p[3]), atof(p[4]), atof(p[5]), atof(p[6]), atof(p[7]));
        return runCalls<complex_t, float>(ops, [&](int n, complex_t* in, float* out) { return b.process(n, in, out); });
    }
    if (mode == "rds" && np == 0) { return runRDS(ops); }

    if (mode == "xlator" && np == 1) {
        auto& b = zeroed<dsp::channel::FrequencyXlator>();
        b.init(NULL, atof(p[0]));
        return runCalls<complex_t, complex_t>(ops, [&](int n, complex_t* in, complex_t* out) { return b.process(n, in, out); },
                                              [&](const Op& op) {
            if (op.kind == 'r') { b.reset(); }
            else if (op.kind == 'w') { b.setOffset(op.v); }
            else { badOp(op); }
        });
    }
    if (mode == "fir_ff" && np == 1) { return runFIR<float, float>(ops, atoi(p[0])); }
    if (mode == "fir_cf" && np == 1) { return runFIR<complex_t, float>(ops, atoi(p[0])); }
    if (mode == "fir_cc" && np == 1) { return runFIR<complex_t, complex_t>(ops, atoi(p[0])); }
    if (mode == "pdec_f" && np == 1) { return runPdec<float>(ops, p); }
    if (mode == "pdec_c" && np == 1) { return runPdec<complex_t>(ops, p); }
    if (mode == "poly_f" && np == 2) { return runPoly<float>(ops, p); }
    if (mode == "poly_c" && np == 2) { return runPoly<complex_t>(ops, p); }
    if (mode == "rres_f" && np == 2) { return runRres<float>(ops, p); }
    if (mode == "rres_c" && np == 2) { return runRres<complex_t>(ops, p); }
    if (mode == "rxvfo" && np == 4) { return runRxVFO(ops, p); }
    if (mode == "quad" && np == 1) {
        auto& b = zeroed<dsp::demod::Quadrature>();
        b.init(NULL, atof(p[0]));
        return runCalls<complex_t, float>(ops, [&](int n, complex_t* in, float* out) { return b.process(n, in, out); },
                                          [&](const Op& op) {
            if (op.kind == 'r') { b.reset(); }
            else if (op.kind == 'v') { b.setDeviation(op.v); }
            else { badOp(op); }
        });
    }
    if (mode == "fm" && np == 4) {
        auto& b = zeroed<dsp::demod::FM<float>>();
        b.init(NULL, atof(p[0]), atof(p[1]), atoi(p[2]) != 0, atoi(p[3]) != 0);
        return runCalls<complex_t, float>(ops, [&](int n, complex_t* in, float* out) { return b.process(n, in, out); },
                                          [&](const Op& op) { if (op.kind == 'r') { b.reset(); } else { badOp(op); } });
    }
    if (mode == "ddc" && np == 2) { return runDDC(ops, p, false); }
    if (mode == "ddcfm" && np == 3) { return runDDC(ops, p, true); }

    if (mode == "am_f" && np == 6) { return runAM<float>(ops, p); }
    if (mode == "am_s" && np == 6) { return runAM<stereo_t>(ops, p); }
    if (mode == "ssb_f" && np == 6) { return runSSB<float>(ops, p); }
    if (mode == "ssb_s" && np == 6) { return runSSB<stereo_t>(ops, p); }
    if (mode == "cw_f" && np == 5) { return runCW<float>(ops, p); }
    if (mode == "cw_s" && np == 5) { return runCW<stereo_t>(ops, p); }
    if (mode == "bfm" && np == 5) { return runBFM(ops, p); }

    if (mode == "pll" && np == 5) { return runPLL<dsp::loop::PLL>(ops, p); }
    if (mode == "cpll" && np == 5) { return runPLL<dsp::loop::CarrierTrackingPLL>(ops, p); }
    if (mode == "mcostas" && np == 6) {
        auto& b = zeroed<dsp::loop::MeteorCostas>();
        b.init(NULL, atof(p[0]), atoi(p[1]) != 0, atof(p[2]), atof(p[3]), atof(p[4]), atof(p[5]));
        return runCalls<complex_t, complex_t>(ops, [&](int n, complex_t* in, complex_t* out) { return b.process(n, in, out); },
                                              [&](const Op& op) {
            if (op.kind == 'r') { b.reset(); }
            else if (op.kind == 'b') { b.setBrokenModulation(op.v != 0); }
            else { badOp(op); }
        });
    }
    if (mode == "meteor" && np == 11) {
        auto& b = zeroed<dsp::demod::Meteor>();
        b.init(NULL, atof(p[0]), atof(p[1]), atoi(p[2]), atof(p[3]), atof(p[4]), atof(p[5]), atoi(p[6]) != 0, atoi(p[7]) != 0,
               atof(p[8]), atof(p[9]), atof(p[10]));
        return runCalls<complex_t, complex_t>(ops, [&](int n, complex_t* in, complex_t* out) { return b.process(n, in, out); },
                                              [&](const Op& op) {
            if (op.kind == 'r') { b.reset(); }
            else if (op.kind == 'b') { b.setBrokenModulation(op.v != 0); }
            else if (op.kind == 'q') { b.setOQPSK(op.a != 0); }
            else { badOp(op); }
        });
    }

    if (mode == "rrc" && np == 3) {
        dsp::tap<float> t = dsp::taps::rootRaisedCosine<float>(atoi(p[0]), atof(p[1]), atof(p[2]));
        fwrite(t.taps, sizeof(float), t.size, stdout);
        return 0;
    }
    if (mode == "mmbank" && np == 2) {
        OpenMM<float>& b = zeroed<OpenMM<float>>();
        b.init(NULL, 4.0, 2.5e-5, 0.01, 0.01, atoi(p[0]), atoi(p[1]));
        auto& bank = b.bank();
        for (int i = 0; i < bank.phaseCount; i++) { fwrite(bank.phases[i], sizeof(float), bank.tapsPerPhase, stdout); }
        return 0;
    }
    if (mode == "fmifwin" && np == 1) {
        OpenFMIF& b = zeroed<OpenFMIF>();
        b.init(NULL, atoi(p[0]));
        fwrite(b.win(), sizeof(float), atoi(p[0]), stdout);
        return 0;
    }
    fprintf(stderr, "ref_blocks: unknown mode or wrong parameter count\n");
    return 2;
}
