"""The IF noise reduction drop-ins against the reference's own block API (CPU only).

Same recipe as test_overlay_syntax.py: the reference's core/src (symlinked into a scratch
directory) gets sdrpp_amd/dsp/gpu/dsp/** copied over it, and a TU that includes the three
noise_reduction headers is compiled with `g++ -fsyntax-only` against the reference's Processor<I,O>,
stream<T> and block. It asserts the base class of each and calls every setter the radio module
calls on them (decoder_modules/radio/src/radio_module.h:73-75, 428, 524, 545, 568). Signatures only:
nothing is linked or run. Skipped where the reference tree is absent (GPU box)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
STUBS = os.path.join(ROOT, "tests", "stubs")
OVERLAY = os.path.join(ROOT, "sdrpp_amd", "dsp", "gpu")

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "core", "src", "dsp")),
                                reason="reference tree not mounted (dev container only)")

TU = """
#include <dsp/noise_reduction/noise_blanker.h>
#include <dsp/noise_reduction/fm_if.h>
#include <dsp/noise_reduction/squelch.h>
#include <type_traits>
using base = dsp::Processor<dsp::complex_t, dsp::complex_t>;
static_assert(std::is_base_of_v<base, dsp::noise_reduction::NoiseBlanker>);
static_assert(std::is_base_of_v<base, dsp::noise_reduction::FMIF>);
static_assert(std::is_base_of_v<base, dsp::noise_reduction::Squelch>);
static_assert(std::is_base_of_v<dsp::block, dsp::noise_reduction::FMIF>);
int main() {
    dsp::noise_reduction::NoiseBlanker nb;
    dsp::noise_reduction::FMIF fmnr;
    dsp::noise_reduction::Squelch squelch;
    nb.init(NULL, 500.0 / 24000.0, 10.0);       // radio_module.h:73
    fmnr.init(NULL, 32);                        // :74
    squelch.init(NULL, -100.0);                 // :75
    nb.setRate(500.0 / 250000.0);               // :428
    nb.setLevel(5.0f);                          // :524 (a float member of the module)
    squelch.setLevel(-50.0f);                   // :545
    fmnr.setBins(15);                           // :568
    nb.reset();
    fmnr.reset();
    dsp::stream<dsp::complex_t> in;
    dsp::noise_reduction::FMIF f2(&in, 9);
    dsp::noise_reduction::NoiseBlanker n2(&in, 0.01, 10.0);
    dsp::noise_reduction::Squelch s2(&in, -40.0);
    dsp::complex_t a[8], b[8];
    int n = fmnr.process(8, a, b) + nb.process(8, a, b) + squelch.process(8, a, b);
    dsp::block* blk[3] = {&nb, &fmnr, &squelch};
    for (auto* p : blk) n += p->run();
    return n + f2.out.read() + n2.out.read() + s2.out.read();
}
"""


def test_ifnr_headers_compile_over_the_reference(tmp_path):
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
    for p in ("noise_reduction/fm_if.h", "noise_reduction/noise_blanker.h", "noise_reduction/squelch.h"):
        assert p in placed and os.path.exists(os.path.join(REF, "core", "src", "dsp", p)), p
    src = tmp_path / "ifnr_overlay.cpp"
    src.write_text(TU)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", str(core), "-I", str(core / "imgui"),
           "-I", STUBS, "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    errs = [ln for ln in r.stderr.splitlines() if "error" in ln]
    assert r.returncode == 0, f"{len(errs)} errors\n" + "\n".join(errs[:40])
