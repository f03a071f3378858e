"""Broadcast-FM banks, the host side (no GPU): the four create functions check every argument before they select
the device, so each refusal (SDRGPU_EARG) shows at device -1 and at device 0 on a machine without one, and valid
arguments at device -1 report the missing device (the form of tests/test_bank_rate_host.py)."""
import ctypes

import numpy as np
import pytest

from sdrpp_amd import lib, F32, C64

EARG, ENODEV = -1, -5
INT_MAX = 2 ** 31 - 1
TAPS = (np.linspace(0.1, 0.8, 8) * np.exp(0.7j * np.arange(8))).astype(np.complex64)
TP = TAPS.ctypes.data_as(ctypes.c_void_p)


def _create(fn, *args):
    h = ctypes.c_void_p()
    return fn(ctypes.byref(h), *args)


# name -> create(device, streams, **changes): valid arguments unless a keyword changes one
def _cfir(dev, streams, dtype=C64, taps=TP, ntaps=8):
    return _create(lib.sdrgpu_bank_fir_complex_create, dev, streams, dtype, taps, ntaps)


def _sdec(dev, streams, fs=240000.0):
    return _create(lib.sdrgpu_bank_stereo_decoder_create, dev, streams, fs)


def _wfm(dev, streams, deviation=100000.0, fs=240000.0, stereo=1, low_pass=1):
    return _create(lib.sdrgpu_bank_broadcast_fm_create, dev, streams, deviation, fs, stereo, low_pass)


def _deemp(dev, streams, tau=50e-6, fs=48000.0):
    return _create(lib.sdrgpu_bank_deemphasis_stereo_create, dev, streams, tau, fs)


CREATES = {"fir_complex": _cfir, "stereo_decoder": _sdec, "broadcast_fm": _wfm, "deemphasis_stereo": _deemp}


@pytest.mark.parametrize("name", sorted(CREATES))
def test_create_without_device(name):
    assert CREATES[name](-1, 65) == ENODEV
    assert b"not available" in lib.sdrgpu_last_error()


def test_every_form_is_valid_without_device():
    assert _cfir(-1, 8, dtype=F32) == ENODEV
    assert _cfir(-1, 8, ntaps=1) == ENODEV
    for stereo in (0, 1):
        for low_pass in (0, 1):
            assert _wfm(-1, 8, stereo=stereo, low_pass=low_pass) == ENODEV, (stereo, low_pass)
    for fs in (120000.0, 240000.0, 250000.0, 384000.0):
        assert _sdec(-1, 8, fs=fs) == ENODEV, fs
        assert _wfm(-1, 8, fs=fs) == ENODEV, fs


@pytest.mark.parametrize("streams", [0, -1, -64, INT_MAX // 64 + 1])
@pytest.mark.parametrize("name", sorted(CREATES))
def test_streams_outside_the_range_are_refused(name, streams):
    assert CREATES[name](-1, streams) == EARG
    assert CREATES[name](0, streams) == EARG


def _no_audio_taps(fs):
    """sdrgpu_broadcast_fm_create designs lowPass(15000, 4000, fs) whether the low-pass runs or not and refuses a
    sample rate at which that design has no tap (3.8 fs / 4000 < 1); the pilot band-pass always has one"""
    return lib.sdrgpu_taps_low_pass(15000.0, 4000.0, fs, 0, None) < 1 and lib.sdrgpu_taps_band_pass_c(18750.0, 19250.0, 3000.0, fs, 1, None) >= 1


@pytest.mark.parametrize("dev", [-1, 0])
def test_argument_checks_need_no_device(dev):
    # element types
    for dtype in (2, -1, 3):
        assert _cfir(dev, 8, dtype=dtype) == EARG, dtype
    # null taps, no taps
    assert _cfir(dev, 8, taps=None) == EARG
    for n in (0, -3):
        assert _cfir(dev, 8, ntaps=n) == EARG
    # history rows x streams beyond INT_MAX: 2^25 streams (the most a bank takes) x 64 history rows = 2^31
    S = INT_MAX // 64
    assert _cfir(dev, S, ntaps=66) == EARG                         # (refused before the taps are read)
    assert _cfir(-1, S, ntaps=8) == ENODEV                         # (7 history rows fit)
    assert _sdec(dev, S) == EARG                                   # 304 history rows of the pilot filter
    assert _wfm(dev, S) == EARG
    assert _wfm(-1, S, stereo=0, low_pass=0) == ENODEV             # (mono without the low-pass keeps no rows)
    # a sample rate or a deviation not > 0
    for fs in (0.0, -240000.0, float("nan")):
        assert _sdec(dev, 8, fs=fs) == EARG, fs
        assert _wfm(dev, 8, fs=fs) == EARG, fs
        assert _deemp(dev, 8, fs=fs) == EARG, fs
        for stereo in (0, 1):
            assert _wfm(dev, 8, fs=fs, stereo=stereo, low_pass=0) == EARG, fs
    for deviation in (0.0, -75000.0, float("nan")):
        assert _wfm(dev, 8, deviation=deviation) == EARG, deviation
    # a sample rate at which the filters cannot be designed: whatever the single-stream block refuses
    for fs in (1.0, 500.0, 1000.0):
        assert _no_audio_taps(fs), fs
        assert _sdec(-1, 8, fs=fs) == ENODEV, fs                   # (the decoder alone has no audio filter)
        for stereo in (0, 1):
            for low_pass in (0, 1):
                assert _wfm(dev, 8, fs=fs, stereo=stereo, low_pass=low_pass) == EARG, (fs, stereo, low_pass)


def test_null_handle_pointers():
    assert lib.sdrgpu_bank_fir_complex_create(None, 0, 4, C64, TP, 8) == EARG
    assert lib.sdrgpu_bank_stereo_decoder_create(None, 0, 4, 240000.0) == EARG
    assert lib.sdrgpu_bank_broadcast_fm_create(None, 0, 4, 100000.0, 240000.0, 1, 1) == EARG
    assert lib.sdrgpu_bank_deemphasis_stereo_create(None, 0, 4, 50e-6, 48000.0) == EARG
