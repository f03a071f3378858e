"""Symbol recovery, the host side (no GPU): taps::rootRaisedCosine and MM's interpolator bank against
numpy restatements, and the argument checks of the new create functions.

* Root raised cosine (taps/root_raised_cosine.h:8-29): an fp64 numpy restatement, one operation per
  reference operation, rounded once to fp32. Bar: 1 ulp of fp32 per tap (the libm's sin / cos may differ
  from numpy's in the last fp64 bit, which can move a tap's single rounding by one fp32 ulp at most).
* Interpolator bank (clock_recovery/mm.h:173-178): windowed_sinc + the layout of buildPolyphaseBank
  (multirate/polyphase_bank.h:32-34), bit-exact.
"""
import ctypes

import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import dsp, lib, F32, C64

EARG, ENODEV = -1, -5


def rrc_restated(count, beta, Ts):
    pi, sqrt2 = 3.14159265358979323846, 1.4142135623730951      # DB_M_PI, DB_M_SQRT2 (math/constants.h:3, 5)
    out = np.empty(count, np.float64)
    half = count / 2.0                                          # :13
    limit = Ts / (4.0 * beta)                                   # :14
    branch = []
    for i in range(count):
        t = float(i) - half + 0.5                               # :16
        if t == 0.0:                                            # :17-19
            out[i] = (1.0 + beta * (4.0 / pi - 1.0)) / Ts
            branch.append("zero")
        elif t == limit or t == -limit:                         # :20-22
            out[i] = ((1.0 + 2.0 / pi) * np.sin(pi / (4.0 * beta)) + (1.0 - 2.0 / pi) * np.cos(pi / (4.0 * beta))) * beta / (Ts * sqrt2)
            branch.append("limit")
        else:                                                   # :23-25
            out[i] = ((np.sin((1.0 - beta) * pi * t / Ts) + np.cos((1.0 + beta) * pi * t / Ts) * 4.0 * beta * t / Ts) /
                      ((1.0 - (4.0 * beta * t / Ts) * (4.0 * beta * t / Ts)) * pi * t / Ts)) / Ts
            branch.append("main")
    return out, branch


@pytest.mark.parametrize("count,beta,Ts,branches", [
    (31, 0.6, 4.0, {"zero", "main"}),
    (32, 0.35, 2.5, {"main"}),
    (17, 0.5, 4.0, {"zero", "limit", "main"}),       # t = +-2 = Ts / (4 beta)
])
def test_root_raised_cosine(count, beta, Ts, branches):
    ref64, branch = rrc_restated(count, beta, Ts)
    assert set(branch) == branches
    if "limit" in branches:
        assert branch.count("limit") == 2
    got = dsp.root_raised_cosine(count, beta, Ts)
    assert got.dtype == np.float32 and got.shape == (count,)
    ref = ref64.astype(np.float32)
    ulp = np.spacing(np.abs(ref))
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / ulp
    print(f"rrc({count}, {beta}, {Ts}): max {err.max():.1f} ulp")
    assert err.max() <= 1.0


def test_root_raised_cosine_arguments():
    assert lib.sdrgpu_taps_root_raised_cosine(31, 0.6, 4.0, None) == 31
    assert lib.sdrgpu_taps_root_raised_cosine(0, 0.6, 4.0, None) == EARG
    assert lib.sdrgpu_taps_root_raised_cosine(31, 0.6, 0.0, None) == EARG


@pytest.mark.parametrize("P,T", [(128, 8), (4, 3)])
def test_mm_interp_bank(P, T):
    lp = dsp.windowed_sinc(P * T, 2.0 * 3.14159265358979323846 * ((0.5 / P) / 1.0), P)   # mm.h:174-175
    ref = np.zeros((P, T), np.float32)
    for i in range(P * T):                                       # polyphase_bank.h:32-34
        ref[(P - 1) - (i % P), i // P] = lp[i]
    got = dsp.mm_interp_bank(P, T)
    assert got.shape == (P, T) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_mm_interp_bank_arguments():
    for P, T in [(0, 8), (1025, 8), (128, 0), (128, 65)]:
        assert lib.sdrgpu_mm_interp_bank(P, T, None) == EARG, (P, T)
    assert lib.sdrgpu_mm_interp_bank(1024, 64, None) == 1024 * 64


def _create(fn, *args):
    h = ctypes.c_void_p()
    return fn(ctypes.byref(h), *args)


PI32 = float(np.float32(3.1415926535))
CREATES = {
    "fast_agc": lambda dev: _create(lib.sdrgpu_fast_agc_create, dev, C64, 1.0, 1e6, 0.1, 1.0),
    "costas": lambda dev: _create(lib.sdrgpu_costas_create, dev, 2, 0.005, 0.0, 0.0, -PI32, PI32),
    "mm": lambda dev: _create(lib.sdrgpu_mm_create, dev, F32, 4.0, 2.5e-5, 0.01, 0.01, 128, 8),
    "binary_slicer": lambda dev: _create(lib.sdrgpu_binary_slicer_create, dev),
    "differential_decoder": lambda dev: _create(lib.sdrgpu_differential_decoder_create, dev, 2, 0),
    "psk": lambda dev: _create(lib.sdrgpu_psk_create, dev, 4, 1.0, 4.0, 31, 0.6, 0.01, 0.005, 2.5e-5, 0.01, 0.01),
    "gfsk": lambda dev: _create(lib.sdrgpu_gfsk_create, dev, 12000.0, 48000.0, 3000.0, 31, 0.6, 2.5e-5, 0.01, 0.01),
    "rds": lambda dev: _create(lib.sdrgpu_rds_create, dev),
}


@pytest.mark.parametrize("name", sorted(CREATES))
def test_create_without_device(name):
    assert CREATES[name](-1) == ENODEV
    assert b"not available" in lib.sdrgpu_last_error()


@pytest.mark.parametrize("args", [
    (F32, 4.0, 2.5e-5, 0.01, 0.01, 0, 8),          # phases outside [1, 1024]
    (F32, 4.0, 2.5e-5, 0.01, 0.01, 1025, 8),
    (F32, 4.0, 2.5e-5, 0.01, 0.01, 128, 0),        # taps per phase outside [1, 64]
    (C64, 4.0, 2.5e-5, 0.01, 0.01, 128, 65),
    (F32, 1.0, 2.5e-5, 0.01, 0.01, 128, 8),        # omega (1 - rel) - muGain = 0.98 < 1
    (C64, 1.02, 1e-6, 0.01, 0.01, 128, 8),         # 1.02 * 0.99 - 0.01 = 0.9998 < 1
    (F32, 4.0, 2.5e-5, 3.0, 0.01, 128, 8),         # 3.96 - 3 < 1
    (7, 4.0, 2.5e-5, 0.01, 0.01, 128, 8),          # no such element type
])
def test_mm_argument_checks_need_no_device(args):
    assert _create(lib.sdrgpu_mm_create, -1, *args) == EARG
    assert _create(lib.sdrgpu_mm_create, 0, *args) == EARG


def test_costas_and_decoder_argument_checks():
    assert _create(lib.sdrgpu_costas_create, -1, 3, 0.005, 0.0, 0.0, -PI32, PI32) == EARG      # static_assert(ORDER ...)
    assert _create(lib.sdrgpu_costas_create, -1, 2, 0.005, 0.0, 0.0, 1.0, 1.0) == EARG         # assert(maxFreq > minFreq)
    assert _create(lib.sdrgpu_differential_decoder_create, -1, 0, 0) == EARG
    assert _create(lib.sdrgpu_fast_agc_create, -1, 2, 1.0, 1e6, 0.1, 1.0) == EARG              # U8 is no sample type
