"""The Meteor demodulator and carrier-loop drop-ins against the reference's own block API (CPU only).

The recipe of test_symsync_overlay.py: the reference's core/src (symlinked into a scratch directory) gets
sdrpp_amd/dsp/gpu/dsp/** copied over it, and its decoder_modules/meteor_demodulator/src (symlinked likewise) gets
sdrpp_amd/dsp/gpu/decoder_modules/meteor_demodulator/src/{meteor_costas.h, meteor_demod.h}. A TU is compiled with
`g++ -fsyntax-only` against the reference's Processor<I,O>, stream<T> and block: it asserts the base class of each
new class, makes every call decoder_modules/meteor_demodulator/src/main.cpp:66, 105, 152, 159 makes on
dsp::demod::Meteor, and calls every setter, reset, process and run of Meteor, MeteorCostas and CarrierTrackingPLL.
Signatures only: nothing is linked or run. Skipped where the reference tree is absent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
STUBS = os.path.join(ROOT, "tests", "stubs")
OVERLAY = os.path.join(ROOT, "sdrpp_amd", "dsp", "gpu")
MODULE = os.path.join("decoder_modules", "meteor_demodulator", "src")

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "core", "src", "dsp")),
                                reason="reference tree not mounted (dev container only)")

TU = """
#include <dsp/loop/carrier_tracking_pll.h>
#include "meteor_costas.h"
#include "meteor_demod.h"
#include <type_traits>
using cc = dsp::Processor<dsp::complex_t, dsp::complex_t>;
static_assert(std::is_base_of_v<cc, dsp::loop::CarrierTrackingPLL>);
static_assert(std::is_base_of_v<cc, dsp::loop::MeteorCostas>);
static_assert(std::is_base_of_v<cc, dsp::demod::Meteor>);
static_assert(std::is_base_of_v<dsp::block, dsp::demod::Meteor>);
#define INPUT_SAMPLE_RATE 150000
int main() {
    dsp::stream<dsp::complex_t> vfoOut;
    bool brokenModulation = false, oqpsk = false;
    // main.cpp:66, 105, 152, 159 (and the setInput / start / stop around them)
    dsp::demod::Meteor demod;
    demod.init(&vfoOut, 72000.0f, INPUT_SAMPLE_RATE, 33, 0.6f, 0.1f, 0.005f, brokenModulation, oqpsk, 1e-6, 0.01);
    demod.start();
    demod.stop();
    demod.setBrokenModulation(brokenModulation);
    demod.setInput(&vfoOut);
    demod.setOQPSK(oqpsk);
    // every setter, reset, process and run
    dsp::complex_t a[8], b[8];
    const dsp::complex_t* ca = a;
    demod.init(&vfoOut, 72000.0, 150000.0, 33, 0.6, 0.1, 0.005, true, true, 1e-6, 0.01, 0.02);
    demod.setSymbolrate(80000.0); demod.setSamplerate(160000.0); demod.setRRCParams(31, 0.5); demod.setRRCTapCount(33);
    demod.setRRCBeta(1); demod.setAGCRate(0.05); demod.setCostasBandwidth(0.01); demod.setMMParams(1e-6, 0.01);
    demod.setMMParams(1e-6, 0.01, 0.02); demod.setOmegaGain(1e-6); demod.setMuGain(0.01); demod.setOmegaRelLimit(0.01);
    demod.reset();
    int n = demod.process(8, ca, b) + demod.run();
    dsp::demod::Meteor d2(&vfoOut, 72000.0, 150000.0, 33, 0.6, 0.1, 0.005, false, true, 1e-6, 0.01);
    dsp::demod::Meteor d3(&vfoOut, 72000.0, 150000.0, 33, 0.6, 0.1, 0.005, false, true, 1e-6, 0.01, 0.01);
    dsp::loop::MeteorCostas mc;
    mc.init(&vfoOut, 0.005, true);
    mc.init(&vfoOut, 0.005, false, 0.0, 0.0, -1.0, 1.0);
    mc.setBrokenModulation(false); mc.setBandwidth(0.01); mc.setInitialPhase(0.1); mc.setInitialFreq(0.2);
    mc.setFrequencyLimits(-1.0, 1.0); mc.reset();
    n += mc.process(8, a, b) + mc.run();
    dsp::loop::MeteorCostas mc2(&vfoOut, 0.005, true, 0.0, 0.0, -1.0, 1.0);
    dsp::loop::CarrierTrackingPLL pll;
    pll.init(&vfoOut, 0.01);
    pll.init(&vfoOut, 0.01, 0.0, 0.0, -1.0, 1.0);
    pll.setBandwidth(0.02); pll.setInitialPhase(0.1); pll.setInitialFreq(0.2); pll.setFrequencyLimits(-1.0, 1.0); pll.reset();
    n += pll.process(8, a, b) + pll.run();
    dsp::loop::CarrierTrackingPLL pll2(&vfoOut, 0.01, 0.0, 0.0, -1.0, 1.0);
    return n + d2.out.read() + d3.out.read() + mc2.out.read() + pll2.out.read();
}
"""


def test_meteor_headers_compile_over_the_reference(tmp_path):
    core, module = tmp_path / "core_src", tmp_path / "meteor_src"
    subprocess.check_call(["cp", "-rs", os.path.join(REF, "core", "src"), str(core)])
    subprocess.check_call(["cp", "-rs", os.path.join(REF, MODULE), str(module)])
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
    assert "loop/carrier_tracking_pll.h" in placed
    assert "loop/pll.h" not in placed, "demod/broadcast_fm.h picks an overlay loop/pll.h up through __has_include"
    for f in ("meteor_costas.h", "meteor_demod.h"):
        assert os.path.exists(os.path.join(REF, MODULE, f)), f
        dst = module / f
        dst.unlink()
        shutil.copyfile(os.path.join(OVERLAY, MODULE, f), dst)
    src = tmp_path / "meteor_overlay.cpp"
    src.write_text(TU)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", str(core), "-I", str(core / "imgui"), "-I", str(module),
           "-I", STUBS, "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    errs = [ln for ln in r.stderr.splitlines() if "error" in ln]
    assert r.returncode == 0, f"{len(errs)} errors\n" + "\n".join(errs[:40])
