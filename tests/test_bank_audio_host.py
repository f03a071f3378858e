"""Analogue receiver banks, the host side (no GPU): every create function checks all its arguments before
it selects the device, so the refusals (SDRGPU_EARG) show on a machine without one, also with a bad
device index, and valid arguments there report the missing device (SDRGPU_ENODEV)."""
import ctypes

import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import lib, dsp, F32, C64

EARG, ENODEV = -1, -5
AGC = (1.0, 50.0 / 48000.0, 5.0 / 48000.0, 10e6, 10.0, float("inf"))


def _create(fn, *args):
    h = ctypes.c_void_p()
    return fn(ctypes.byref(h), *args)


# name -> create(device, streams, **changes): valid arguments unless a keyword changes one
def _agc(dev, streams, dtype=C64, enabled=1):
    return _create(lib.sdrgpu_bank_agc_create, dev, streams, dtype, *AGC, enabled)


def _dcb(dev, streams, dtype=F32):
    return _create(lib.sdrgpu_bank_dc_blocker_create, dev, streams, dtype, 1e-3)


def _deemp(dev, streams, samplerate=48000.0):
    return _create(lib.sdrgpu_bank_deemphasis_create, dev, streams, 50e-6, samplerate)


def _squelch(dev, streams):
    return _create(lib.sdrgpu_bank_squelch_create, dev, streams, -30.0)


def _fm(dev, streams, samplerate=48000.0, bandwidth=12500.0, flags=(1, 0)):
    return _create(lib.sdrgpu_bank_fm_create, dev, streams, samplerate, bandwidth, *flags)


def _am(dev, streams, mode=1, bandwidth=10000.0, samplerate=48000.0):
    return _create(lib.sdrgpu_bank_am_create, dev, streams, mode, bandwidth, AGC[1], AGC[2], 1e-3, samplerate)


CREATES = {"agc": _agc, "dc_blocker": _dcb, "deemphasis": _deemp, "squelch": _squelch, "fm": _fm, "am": _am}
BAD_DEVICES = [-1, 1 << 20]


@pytest.mark.parametrize("dev", BAD_DEVICES)
@pytest.mark.parametrize("name", sorted(CREATES))
def test_create_without_device(name, dev):
    assert CREATES[name](dev, 65) == ENODEV
    assert b"not available" in lib.sdrgpu_last_error()


@pytest.mark.parametrize("streams", [0, -1, -64])
@pytest.mark.parametrize("name", sorted(CREATES))
def test_streams_below_one_are_refused(name, streams):
    for dev in BAD_DEVICES + [0]:
        assert CREATES[name](dev, streams) == EARG


@pytest.mark.parametrize("dev", BAD_DEVICES + [0])
def test_argument_checks_need_no_device(dev):
    # element types
    for dtype in (2, -1, 7):
        assert _agc(dev, 8, dtype=dtype) == EARG
        assert _agc(dev, 8, dtype=dtype, enabled=0) == EARG
        assert _dcb(dev, 8, dtype=dtype) == EARG
    # agcMode outside 0..2
    for mode in (-1, 3):
        assert _am(dev, 8, mode=mode) == EARG
    # sample rates and bandwidths
    for bad in (0.0, -48000.0, float("nan")):
        assert _deemp(dev, 8, samplerate=bad) == EARG
        assert _fm(dev, 8, samplerate=bad) == EARG
        assert _fm(dev, 8, bandwidth=bad) == EARG
        assert _fm(dev, 8, bandwidth=bad, flags=(0, 0)) == EARG
        for mode in (0, 1, 2):
            assert _am(dev, 8, mode=mode, samplerate=bad) == EARG
            assert _am(dev, 8, mode=mode, bandwidth=bad) == EARG


def test_valid_modes_reach_the_device_check():
    for mode in (0, 1, 2):
        assert _am(-1, 8, mode=mode) == ENODEV
    for flags in ((0, 0), (1, 0), (0, 1), (1, 1)):
        assert _fm(-1, 8, flags=flags) == ENODEV
    for dtype in (F32, C64):
        assert _agc(-1, 8, dtype=dtype, enabled=0) == ENODEV
        assert _dcb(-1, 8, dtype=dtype) == ENODEV


def test_null_handles():
    assert lib.sdrgpu_bank_agc_set_gain(None, 1.0) == EARG
    assert lib.sdrgpu_bank_squelch_muted(None, None) == EARG
    assert lib.sdrgpu_bank_agc_create(None, 0, 4, C64, *AGC, 1) == EARG
    assert lib.sdrgpu_bank_dc_blocker_create(None, 0, 4, F32, 1e-3) == EARG
    assert lib.sdrgpu_bank_deemphasis_create(None, 0, 4, 50e-6, 48000.0) == EARG
    assert lib.sdrgpu_bank_squelch_create(None, 0, 4, -30.0) == EARG
    assert lib.sdrgpu_bank_fm_create(None, 0, 4, 48000.0, 12500.0, 1, 0) == EARG
    assert lib.sdrgpu_bank_am_create(None, 0, 4, 1, 10000.0, AGC[1], AGC[2], 1e-3, 48000.0) == EARG


def _without_handle(cls, streams, in_dtype):
    """A bank object with no handle: process() checks the shape before it touches one."""
    b = cls.__new__(cls)
    b._h, b.streams, b.in_dtype, b.out_dtype = None, streams, in_dtype, np.float32
    return b


@pytest.mark.parametrize("cls,dt", [(dsp.BankAGC, np.float32), (dsp.BankDCBlocker, np.float32), (dsp.BankDeemphasis, np.float32),
                                    (dsp.BankSquelch, np.complex64), (dsp.BankFM, np.complex64), (dsp.BankAM, np.complex64)])
def test_python_classes_refuse_a_wrong_shape(cls, dt):
    b = _without_handle(cls, 5, dt)
    for shape in [(7, 4), (7, 6), (35,), (7, 5, 1)]:
        with pytest.raises(ValueError):
            b.process(np.zeros(shape, dt))
    with pytest.raises(sdrpp_amd.SdrGpuError):                  # the right shape passes the check (and then finds no handle)
        b.process(np.zeros((7, 5), dt))
