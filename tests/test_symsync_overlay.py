"""The symbol recovery drop-ins against the reference's own block API (CPU only).

Same recipe as test_ifnr_overlay.py: the reference's core/src (symlinked into a scratch directory) gets
sdrpp_amd/dsp/gpu/dsp/** copied over it, and a TU that includes the seven new headers is compiled with
`g++ -fsyntax-only` against the reference's Processor<I,O>, stream<T> and block. It asserts the base
class of each, makes every call decoder_modules/radio/src/demodulators/wfm.h:57-68 makes on them, and
calls init, every setter, reset, process and run of PSK<4> and GFSK. Signatures only: nothing is linked
or run. Skipped where the reference tree is absent (GPU box)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
STUBS = os.path.join(ROOT, "tests", "stubs")
OVERLAY = os.path.join(ROOT, "sdrpp_amd", "dsp", "gpu")
HEADERS = ("loop/fast_agc.h", "loop/costas.h", "clock_recovery/mm.h", "digital/binary_slicer.h",
           "digital/differential_decoder.h", "demod/psk.h", "demod/gfsk.h")

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "core", "src", "dsp")),
                                reason="reference tree not mounted (dev container only)")

TU = """
#include <dsp/loop/fast_agc.h>
#include <dsp/loop/costas.h>
#include <dsp/clock_recovery/mm.h>
#include <dsp/digital/binary_slicer.h>
#include <dsp/digital/differential_decoder.h>
#include <dsp/demod/psk.h>
#include <dsp/demod/gfsk.h>
#include <dsp/taps/band_pass.h>
#include <dsp/filter/fir.h>
#include <dsp/convert/complex_to_real.h>
#include <dsp/math/hz_to_rads.h>
#include <type_traits>
using cc = dsp::Processor<dsp::complex_t, dsp::complex_t>;
static_assert(std::is_base_of_v<cc, dsp::loop::FastAGC<dsp::complex_t>>);
static_assert(std::is_base_of_v<dsp::Processor<float, float>, dsp::loop::FastAGC<float>>);
static_assert(std::is_base_of_v<cc, dsp::loop::Costas<2>>);
static_assert(std::is_base_of_v<cc, dsp::loop::Costas<8>>);
static_assert(std::is_base_of_v<dsp::Processor<float, float>, dsp::clock_recovery::MM<float>>);
static_assert(std::is_base_of_v<cc, dsp::clock_recovery::MM<dsp::complex_t>>);
static_assert(std::is_base_of_v<dsp::Processor<float, uint8_t>, dsp::digital::BinarySlicer>);
static_assert(std::is_base_of_v<dsp::Processor<uint8_t, uint8_t>, dsp::digital::DifferentialDecoder>);
static_assert(std::is_base_of_v<cc, dsp::demod::PSK<4>>);
static_assert(std::is_base_of_v<dsp::Processor<dsp::complex_t, float>, dsp::demod::GFSK>);
static_assert(std::is_base_of_v<dsp::block, dsp::demod::GFSK>);
int main() {
    // wfm.h:104-113 members, :57-68 calls
    dsp::stream<dsp::complex_t> rdsOut;
    dsp::loop::FastAGC<dsp::complex_t> agc;
    dsp::loop::Costas<2> costas, costas2;
    dsp::tap<dsp::complex_t> taps;
    dsp::filter::FIR<dsp::complex_t, dsp::complex_t> fir;
    dsp::convert::ComplexToReal c2r;
    dsp::clock_recovery::MM<float> recov;
    dsp::digital::BinarySlicer slice;
    dsp::digital::DifferentialDecoder diff;
    agc.init(&rdsOut, 1.0, 1e6, 0.1);
    costas.init(&agc.out, 0.005f);
    taps = dsp::taps::bandPass<dsp::complex_t>(0, 2375, 100, 5000);
    fir.init(&costas.out, taps);
    double baudfreq = dsp::math::hzToRads(2375.0 / 2.0, 5000);
    costas2.init(&fir.out, 0.01, 0.0, baudfreq, baudfreq - (baudfreq * 0.1), baudfreq + (baudfreq * 0.1));
    c2r.init(&costas2.out);
    recov.init(&c2r.out, 5000.0 / (2375.0 / 2.0), 1e-6, 0.01, 0.01);
    slice.init(&recov.out);
    diff.init(&slice.out, 2);
    dsp::block* chain[6] = {&agc, &costas, &costas2, &recov, &slice, &diff};
    int n = 0;
    for (auto* b : chain) { b->start(); b->stop(); n += b->run(); }
    // every setter of the five blocks
    agc.setSetPoint(1.0); agc.setMaxGain(1e6); agc.setRate(0.1); agc.setInitGain(1.0); agc.setGain(2.0); agc.reset();
    dsp::loop::FastAGC<float> fagc(&recov.out, 1.0, 10.0, 0.01, 1.0);
    costas.setBandwidth(0.01); costas.setInitialPhase(0.1); costas.setInitialFreq(0.2); costas.setFrequencyLimits(-1.0, 1.0); costas.reset();
    dsp::loop::Costas<4> c4(&rdsOut, 0.005, 0.0, 0.0, -1.0, 1.0);
    dsp::loop::Costas<8> c8(&rdsOut, 0.005);
    recov.setOmega(4.0); recov.setOmegaGain(1e-6); recov.setMuGain(0.01); recov.setOmegaRelLimit(0.01); recov.setInterpParams(64, 8); recov.reset();
    dsp::clock_recovery::MM<dsp::complex_t> cm(&rdsOut, 4.0, 2.5e-5, 0.01, 0.01, 128, 8);
    diff.setModulus(4); diff.setInitSym(1); diff.reset();
    dsp::digital::BinarySlicer s2(&recov.out);
    dsp::digital::DifferentialDecoder d2(&slice.out);
    dsp::complex_t a[8], b[8];
    float fa[8], fb[8];
    uint8_t ua[8], ub[8];
    n += agc.process(8, a, b) + costas.process(8, a, b) + recov.process(8, fa, fb) + cm.process(8, a, b);
    n += slice.process(8, fa, ua) + diff.process(8, ua, ub) + fagc.process(8, fa, fb);
    // PSK<4> and GFSK: init, all setters, reset, process, run
    dsp::demod::PSK<4> psk;
    psk.init(&rdsOut, 72000.0, 144000.0, 31, 0.6, 0.01, 0.005, 2.5e-5, 0.01);
    psk.init(&rdsOut, 72000.0, 144000.0, 31, 0.6, 0.01, 0.005, 2.5e-5, 0.01, 0.01);
    psk.setSymbolrate(36000.0); psk.setSamplerate(144000.0); psk.setRRCParams(33, 0.5); psk.setRRCTapCount(31); psk.setRRCBeta(1);
    psk.setAGCRate(0.02); psk.setCostasBandwidth(0.01); psk.setMMParams(1e-6, 0.01); psk.setMMParams(1e-6, 0.01, 0.02);
    psk.setOmegaGain(1e-6); psk.setMuGain(0.01); psk.setOmegaRelLimit(0.01); psk.reset();
    n += psk.process(8, a, b) + psk.run();
    dsp::demod::PSK<2> p2(&rdsOut, 1200.0, 4800.0, 31, 0.6, 0.01, 0.005, 2.5e-5, 0.01, 0.01);
    dsp::demod::GFSK gfsk;
    gfsk.init(&rdsOut, 4800.0, 19200.0, 2400.0, 31, 0.6, 2.5e-5, 0.01);
    gfsk.init(&rdsOut, 4800.0, 19200.0, 2400.0, 31, 0.6, 2.5e-5, 0.01, 0.01);
    gfsk.setSymbolrate(2400.0); gfsk.setSamplerate(19200.0); gfsk.setDeviation(1200.0); gfsk.setRRCParams(33, 0.5);
    gfsk.setRRCTapCount(31); gfsk.setRRCBeta(1); gfsk.setMMParams(1e-6, 0.01); gfsk.setMMParams(1e-6, 0.01, 0.02);
    gfsk.setOmegaGain(1e-6); gfsk.setMuGain(0.01); gfsk.setOmegaRelLimit(0.01); gfsk.reset();
    n += gfsk.process(8, a, fb) + gfsk.run();
    dsp::demod::GFSK g2(&rdsOut, 4800.0, 19200.0, 2400.0, 31, 0.6, 2.5e-5, 0.01, 0.01);
    return n + p2.out.read() + g2.out.read() + s2.out.read() + d2.out.read() + c4.out.read() + c8.out.read() + cm.out.read();
}
"""


def test_symsync_headers_compile_over_the_reference(tmp_path):
    core = tmp_path / "core_src"
    subprocess.check_call(["cp", "-rs", os.path.join(REF, "core", "src"), str(core)])
    placed = []
    for dp, _, fn in os.walk(os.path.join(OVERLAY, "dsp")):
        for f in fn:
            rel = os.path.relpath(os.path.join(dp, f), os.path.join(OVERLAY, "dsp"))
            dst = core / "dsp" / rel
            dst.parent.mkdir(parents=True, exist_ok=True)
            if dst.is_symlink() or dst.exists():
                dst.unlink()
            shutil.copyfile(os.path.join(dp, f), dst)
            placed.append(rel)
    for p in HEADERS:
        assert p in placed and os.path.exists(os.path.join(REF, "core", "src", "dsp", p)), p
    src = tmp_path / "symsync_overlay.cpp"
    src.write_text(TU)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", str(core), "-I", str(core / "imgui"),
           "-I", STUBS, "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    errs = [ln for ln in r.stderr.splitlines() if "error" in ln]
    assert r.returncode == 0, f"{len(errs)} errors\n" + "\n".join(errs[:40])
