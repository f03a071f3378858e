"""Rate-changing banks, the host side (no GPU): the four create functions check every argument before
they select the device, so each refusal (SDRGPU_EARG) shows at device -1 and at device 0 on a machine
without one, and valid arguments at device -1 report the missing device (the form of tests/test_banks_host.py)."""
import ctypes

import numpy as np
import pytest

from sdrpp_amd import lib, F32, C64

EARG, ENODEV = -1, -5
INT_MAX = 2 ** 31 - 1
TAPS = np.linspace(0.1, 0.8, 8).astype(np.float32)
TP = TAPS.ctypes.data_as(ctypes.c_void_p)


def _create(fn, *args):
    h = ctypes.c_void_p()
    return fn(ctypes.byref(h), *args)


# name -> create(device, streams, **changes): valid arguments unless a keyword changes one
def _dfir(dev, streams, dtype=C64, taps=TP, ntaps=8, decim=2):
    return _create(lib.sdrgpu_bank_decimating_fir_create, dev, streams, dtype, taps, ntaps, decim)


def _poly(dev, streams, dtype=C64, interp=4, decim=5, taps=TP, ntaps=8):
    return _create(lib.sdrgpu_bank_polyphase_resampler_create, dev, streams, dtype, interp, decim, taps, ntaps)


def _pdec(dev, streams, dtype=C64, ratio=4):
    return _create(lib.sdrgpu_bank_power_decimator_create, dev, streams, dtype, ratio)


def _rres(dev, streams, dtype=F32, rates=(25000.0, 8000.0)):
    return _create(lib.sdrgpu_bank_rational_resampler_create, dev, streams, dtype, *rates)


CREATES = {"decimating_fir": _dfir, "polyphase": _poly, "power_decimator": _pdec, "rational": _rres}


@pytest.mark.parametrize("name", sorted(CREATES))
def test_create_without_device(name):
    assert CREATES[name](-1, 65) == ENODEV
    assert b"not available" in lib.sdrgpu_last_error()


def test_every_plan_mode_is_valid_without_device():
    for rates in [(25000.0, 8000.0), (32000.0, 8000.0), (10000.0, 8000.0), (8000.0, 8000.0), (8000.0, 12000.0)]:
        for dtype in (F32, C64):
            assert _rres(-1, 8, dtype=dtype, rates=rates) == ENODEV, rates
    for ratio in (1, 2, 8192):
        assert _pdec(-1, 8, ratio=ratio) == ENODEV, ratio
    assert _poly(-1, 8, interp=16, ntaps=5) == ENODEV               # fewer taps than phases
    assert _poly(-1, 8, interp=3, ntaps=8) == ENODEV                # ntaps % interp != 0


@pytest.mark.parametrize("streams", [0, -1, -64])
@pytest.mark.parametrize("name", sorted(CREATES))
def test_streams_below_one_are_refused(name, streams):
    assert CREATES[name](-1, streams) == EARG
    assert CREATES[name](0, streams) == EARG


@pytest.mark.parametrize("dev", [-1, 0])
def test_argument_checks_need_no_device(dev):
    # element types
    for name in sorted(CREATES):
        assert CREATES[name](dev, 8, dtype=2) == EARG, name
        assert CREATES[name](dev, 8, dtype=-1) == EARG, name
    # null taps, no taps
    assert _dfir(dev, 8, taps=None) == EARG
    assert _poly(dev, 8, taps=None) == EARG
    for n in (0, -3):
        assert _dfir(dev, 8, ntaps=n) == EARG
        assert _poly(dev, 8, ntaps=n) == EARG
    # interp < 1, decim < 1
    for v in (0, -2):
        assert _dfir(dev, 8, decim=v) == EARG
        assert _poly(dev, 8, decim=v) == EARG
        assert _poly(dev, 8, interp=v) == EARG
    # a ratio sdrgpu_decim_plan refuses
    for ratio in (0, -2, 3, 6, 16384):
        assert _pdec(dev, 8, ratio=ratio) == EARG, ratio
    # a sample rate not > 0
    for rates in [(0.0, 8000.0), (25000.0, 0.0), (-1.0, 8000.0), (25000.0, -8000.0), (float("nan"), 8000.0)]:
        assert _rres(dev, 8, rates=rates) == EARG, rates
    # history rows x streams beyond INT_MAX: 2^25 streams (the most a bank takes) x 64 history rows = 2^31
    S = INT_MAX // 64
    assert _dfir(dev, S, ntaps=66) == EARG                         # (refused before the taps are read)
    assert _poly(dev, S, interp=1, ntaps=66) == EARG
    assert _poly(dev, S, interp=2, ntaps=131) == EARG              # 66 taps per phase
    assert _dfir(-1, S, ntaps=8) == ENODEV                         # (7 history rows fit)
    # interp x taps-per-phase beyond INT_MAX: 2^30 + 1 phases of ceil((2^30 + 2) / (2^30 + 1)) = 2 taps
    assert _poly(dev, 1, interp=2 ** 30 + 1, ntaps=2 ** 30 + 2) == EARG
    # streams beyond what a bank takes
    assert _dfir(dev, INT_MAX // 64 + 1) == EARG


def test_null_handle_pointers():
    assert lib.sdrgpu_bank_decimating_fir_create(None, 0, 4, C64, TP, 8, 2) == EARG
    assert lib.sdrgpu_bank_polyphase_resampler_create(None, 0, 4, C64, 4, 5, TP, 8) == EARG
    assert lib.sdrgpu_bank_power_decimator_create(None, 0, 4, C64, 4) == EARG
    assert lib.sdrgpu_bank_rational_resampler_create(None, 0, 4, C64, 25000.0, 8000.0) == EARG
