"""The host side of what tests/test_ref_demod.py made the device follow (no GPU):
* the drop-in BroadcastFM's setRDSOut (sdrpp_amd/dsp/gpu/dsp/demod/broadcast_fm.h), compiled over the reference's
  Processor / stream headers and run against a C ABI that only records its calls: on a handle that has the RDS
  branch, setRDSOut is sdrgpu_broadcast_fm_set_rds followed by sdrgpu_block_reset on the SAME handle (the
  reference's setRDSOut is the flag and reset(), which keeps the RDS branch's xlator phase and resampler history;
  a rebuilt handle would lose them); on the mono handle, which has no RDS branch and has run none, it builds the
  full handle. Skipped where the reference tree is absent;
* the setters the op lists use refuse a null handle.
"""
import os
import subprocess

import pytest

from sdrpp_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
EARG, ESTATE = -1, -4

PROGRAM = r"""
#include <cstdio>
#include <dsp/demod/broadcast_fm.h>
// a C ABI that records: handles are numbered in the order they are created
static int made = 0;
static long id(sdrgpu_block* h) { return (long)(size_t)h; }
extern "C" {
int sdrgpu_broadcast_fm_create(sdrgpu_block** h, int, double, double, int stereo, int) { *h = (sdrgpu_block*)(size_t)++made; printf("create_full %d stereo=%d\n", made, stereo); return 0; }
int sdrgpu_wfm_create(sdrgpu_block** h, int, double, double, int) { *h = (sdrgpu_block*)(size_t)++made; printf("create_mono %d\n", made); return 0; }
int sdrgpu_broadcast_fm_set_rds(sdrgpu_block* h, int on) { printf("set_rds %ld %d\n", id(h), on); return 0; }
int sdrgpu_block_reset(sdrgpu_block* h) { printf("reset %ld\n", id(h)); return 0; }
int sdrgpu_block_destroy(sdrgpu_block* h) { printf("destroy %ld\n", id(h)); return 0; }
const char* sdrgpu_last_error(void) { return ""; }
int sdrgpu_device_count(void) { return 1; }
}
int main() {
    {
        dsp::demod::BroadcastFM b;
        b.init(NULL, 100000.0, 240000.0, true, true, true);
        puts("-- stereo with RDS: off, on");
        b.setRDSOut(false);
        b.setRDSOut(true);
        puts("-- reset");
        b.reset();
    }
    {
        dsp::demod::BroadcastFM b;
        b.init(NULL, 100000.0, 240000.0, false, true, false);
        puts("-- mono without RDS: on, off, on");
        b.setRDSOut(true);
        b.setRDSOut(false);
        b.setRDSOut(true);
    }
    return 0;
}
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "core", "src", "dsp")), reason="reference tree not mounted (dev container only)")
def test_drop_in_set_rds_out_is_the_flag_and_a_reset_of_the_same_handle(tmp_path):
    core = tmp_path / "core_src"
    subprocess.check_call(["cp", "-rs", os.path.join(REF, "core", "src"), str(core)])
    overlay = os.path.join(ROOT, "sdrpp_amd", "dsp", "gpu", "dsp")
    for dp, _, fn in os.walk(overlay):
        for f in fn:
            dst = core / "dsp" / os.path.relpath(os.path.join(dp, f), overlay)
            dst.parent.mkdir(parents=True, exist_ok=True)
            if dst.is_symlink() or dst.exists():
                dst.unlink()
            dst.write_bytes(open(os.path.join(dp, f), "rb").read())
    src, exe = tmp_path / "set_rds_out.cpp", tmp_path / "set_rds_out"
    src.write_text(PROGRAM)
    # the host runtime's symbols (flog, threading) and VOLK come from the reference probe's stand-ins; C-ABI
    # functions that the included drop-in headers name but this program never calls stay unresolved
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-w", "-I", str(core), "-I", os.path.join(ROOT, "oracle", "ref_fmt"),
                           "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                           os.path.join(ROOT, "oracle", "ref_standins.cpp"), "-o", str(exe), "-lpthread",
                           "-Wl,--unresolved-symbols=ignore-all"], timeout=600)
    log = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    print("\n".join(log))
    at = log.index("-- stereo with RDS: off, on")
    assert log[:at] == ["create_full 1 stereo=1", "set_rds 1 1"]
    assert log[at + 1:at + 5] == ["set_rds 1 0", "reset 1", "set_rds 1 1", "reset 1"]      # no handle is built or destroyed
    assert log[at + 5:at + 8] == ["-- reset", "reset 1", "destroy 1"]
    at = log.index("-- mono without RDS: on, off, on")
    assert log[at - 1] == "create_mono 2"
    # on: the mono handle has no RDS branch, the full one is built; from then on the handle is kept
    assert log[at + 1:at + 4] == ["create_full 3 stereo=0", "set_rds 3 1", "destroy 2"]
    assert log[at + 4:at + 8] == ["set_rds 3 0", "reset 3", "set_rds 3 1", "reset 3"]
    assert [ln for ln in log[at + 8:] if ln] == ["destroy 3"]


def test_the_setters_refuse_a_null_handle():
    assert lib.sdrgpu_demod_agc_set_attack_decay(None, 0.01, 0.001) == EARG
    assert lib.sdrgpu_demod_agc_set_enabled(None, 0, 1) == ESTATE and lib.sdrgpu_demod_agc_set_gain(None, 0, 2.0) == ESTATE
    assert lib.sdrgpu_dc_blocker_set_rate(None, 0.002) == ESTATE
    assert lib.sdrgpu_broadcast_fm_set_rds(None, 1) == EARG
    assert lib.sdrgpu_block_reset(None) == EARG
    assert lib.sdrgpu_cw_set_tone(None, 700.0) == EARG
