// The reference's Meteor demodulator and carrier loops, run from its own headers (included by path, nothing
// of them is copied here): the program behind tests/golden/ref_meteor_*.npz. tools/gen_meteor_fixtures.py
// compiles it into a temporary directory with the reference tree, oracle/ref_fmt and tests/stubs on the
// include path, links oracle/ref_standins.cpp, and runs it.
//
//   ref_meteor_probe MODE CALLS PARAMS... < samples (complex64) > int32 n, int32 counts[n], complex64 outputs
//
// MODE and PARAMS (every block's init order):
//   pll      bandwidth initPhase initFreq minFreq maxFreq                  loop::PLL
//   cpll     bandwidth initPhase initFreq minFreq maxFreq                  loop::CarrierTrackingPLL
//   mcostas  bandwidth broken initPhase initFreq minFreq maxFreq           loop::MeteorCostas
//   meteor   symbolrate samplerate rrcTaps rrcBeta agcRate costasBw broken oqpsk omegaGain muGain omegaRelLimit
// CALLS, comma separated: a sample count is one process() call of that many samples (n of the output counts
// them); r = reset(); b0 / b1 = setBrokenModulation; q0 / q1 = setOQPSK.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <new>
#include <string>
#include <vector>
#include <dsp/loop/pll.h>
#include <dsp/loop/carrier_tracking_pll.h>
#include "meteor_demod.h"

using dsp::complex_t;

struct Call {
    char kind = 'p';   // 'p' process, 'r' reset, 'b' setBrokenModulation, 'q' setOQPSK
    int arg = 0;       // the sample count, or the flag
};

static std::vector<Call> parse(const std::string& s) {
    std::vector<Call> calls;
    for (size_t at = 0; at <= s.size();) {
        size_t end = s.find(',', at);
        if (end == std::string::npos) { end = s.size(); }
        const std::string tok = s.substr(at, end - at);
        at = end + 1;
        if (tok.empty()) { continue; }
        Call c;
        if (tok[0] == 'r') { c.kind = 'r'; }
        else if (tok[0] == 'b' || tok[0] == 'q') { c.kind = tok[0]; c.arg = atoi(tok.c_str() + 1); }
        else { c.arg = atoi(tok.c_str()); }
        calls.push_back(c);
    }
    return calls;
}

// A block in zero-filled storage, as one of static storage duration would be. Never destroyed: the process ends.
template <class T>
static T& zeroed() {
    return *new (calloc(1, sizeof(T))) T();
}

static int run(const std::vector<Call>& calls, const std::function<int(int, complex_t*, complex_t*)>& process,
               const std::function<void(const Call&)>& other) {
    size_t total = 0;
    for (const Call& c : calls) { total += c.kind == 'p' ? c.arg : 0; }
    std::vector<complex_t> x(total + 1), y(total + calls.size() + 1);
    if (fread(x.data(), sizeof(complex_t), total, stdin) != total) { fprintf(stderr, "ref_meteor_probe: short input\n"); return 3; }
    std::vector<int32_t> counts;
    size_t in = 0, out = 0;
    for (const Call& c : calls) {
        if (c.kind != 'p') { other(c); continue; }
        const int n = process(c.arg, x.data() + in, y.data() + out);
        counts.push_back(n);
        in += c.arg;
        out += n;
    }
    const int32_t nc = (int32_t)counts.size();
    fwrite(&nc, sizeof(nc), 1, stdout);
    fwrite(counts.data(), sizeof(int32_t), counts.size(), stdout);
    fwrite(y.data(), sizeof(complex_t), out, stdout);
    return 0;
}

static int usage() {
    fprintf(stderr, "ref_meteor_probe: pll | cpll | mcostas | meteor, CALLS, PARAMS (see the file's head)\n");
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 3) { return usage(); }
    const std::string mode = argv[1];
    const std::vector<Call> calls = parse(argv[2]);
    char** p = argv + 3;
    const int np = argc - 3;
    auto num = [&](int i) { return atof(p[i]); };
    if ((mode == "pll" || mode == "cpll") && np == 5) {
        if (mode == "pll") {
            auto& b = zeroed<dsp::loop::PLL>();
            b.init(NULL, num(0), num(1), num(2), num(3), num(4));
            return run(calls, [&](int n, complex_t* in, complex_t* out) { return b.process(n, in, out); },
                       [&](const Call& c) { if (c.kind == 'r') { b.reset(); } });
        }
        auto& b = zeroed<dsp::loop::CarrierTrackingPLL>();
        b.init(NULL, num(0), num(1), num(2), num(3), num(4));
        return run(calls, [&](int n, complex_t* in, complex_t* out) { return b.process(n, in, out); },
                   [&](const Call& c) { if (c.kind == 'r') { b.reset(); } });
    }
    if (mode == "mcostas" && np == 6) {
        auto& b = zeroed<dsp::loop::MeteorCostas>();
        b.init(NULL, num(0), atoi(p[1]) != 0, num(2), num(3), num(4), num(5));
        return run(calls, [&](int n, complex_t* in, complex_t* out) { return b.process(n, in, out); },
                   [&](const Call& c) {
                       if (c.kind == 'r') { b.reset(); }
                       if (c.kind == 'b') { b.setBrokenModulation(c.arg != 0); }
                   });
    }
    if (mode == "meteor" && np == 11) {
        auto& b = zeroed<dsp::demod::Meteor>();
        b.init(NULL, num(0), num(1), atoi(p[2]), num(3), num(4), num(5), atoi(p[6]) != 0, atoi(p[7]) != 0, num(8), num(9), num(10));
        return run(calls, [&](int n, complex_t* in, complex_t* out) { return b.process(n, in, out); },
                   [&](const Call& c) {
                       if (c.kind == 'r') { b.reset(); }
                       if (c.kind == 'b') { b.setBrokenModulation(c.arg != 0); }
                       if (c.kind == 'q') { b.setOQPSK(c.arg != 0); }
                   });
    }
    return usage();
}
