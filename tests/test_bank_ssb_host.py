"""SSB and CW receiver banks, the bank xlator and the single-stream CW block, the host side (no GPU): every
create function checks all its arguments before it selects the device, so the refusals (SDRGPU_EARG) show on
a machine without one, also with a bad device index, and valid arguments there report the missing device
(SDRGPU_ENODEV)."""
import ctypes

import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import lib, dsp

EARG, ENODEV = -1, -5
FS = 24000.0
ATTACK, DECAY = 50.0 / FS, 5.0 / FS
NAN, INF = float("nan"), float("inf")


def _create(fn, *args):
    h = ctypes.c_void_p()
    return fn(ctypes.byref(h), *args)


# name -> create(device, streams, **changes): valid arguments unless a keyword changes one
def _xlator(dev, streams, offset=0.3):
    return _create(lib.sdrgpu_bank_xlator_create, dev, streams, offset)


def _xlator_real(dev, streams, offset=0.3):
    return _create(lib.sdrgpu_bank_xlator_real_create, dev, streams, offset)


def _ssb(dev, streams, mode=0, bandwidth=2800.0, samplerate=FS, agc=1):
    return _create(lib.sdrgpu_bank_ssb_create, dev, streams, mode, bandwidth, samplerate, agc, ATTACK, DECAY)


def _bank_cw(dev, streams, tone=800.0, samplerate=FS, agc=1):
    return _create(lib.sdrgpu_bank_cw_create, dev, streams, tone, agc, ATTACK, DECAY, samplerate)


def _cw(dev, streams=None, tone=800.0, samplerate=FS, agc=1, stereo=0):
    """(single stream: `streams` is not an argument)"""
    return _create(lib.sdrgpu_cw_create, dev, tone, agc, ATTACK, DECAY, samplerate, stereo)


BANKS = {"xlator": _xlator, "xlator_real": _xlator_real, "ssb": _ssb, "cw": _bank_cw}
CREATES = dict(BANKS, single_cw=_cw)
BAD_DEVICES = [-1, 1 << 20]
DEVICES = BAD_DEVICES + [0]


@pytest.mark.parametrize("dev", BAD_DEVICES)
@pytest.mark.parametrize("name", sorted(CREATES))
def test_create_without_device(name, dev):
    assert CREATES[name](dev, 65) == ENODEV
    assert b"not available" in lib.sdrgpu_last_error()


@pytest.mark.parametrize("streams", [0, -1])
@pytest.mark.parametrize("name", sorted(BANKS))
def test_streams_below_one_are_refused(name, streams):
    for dev in DEVICES:
        assert BANKS[name](dev, streams) == EARG


@pytest.mark.parametrize("dev", DEVICES)
def test_argument_checks_need_no_device(dev):
    for mode in (-1, 3):
        assert _ssb(dev, 8, mode=mode) == EARG
        assert _ssb(dev, 8, mode=mode, agc=0) == EARG
    for bad in (0.0, -1.0, INF, NAN):
        for mode in (0, 1, 2):
            assert _ssb(dev, 8, mode=mode, samplerate=bad) == EARG
        assert _bank_cw(dev, 8, samplerate=bad) == EARG
        assert _cw(dev, samplerate=bad) == EARG
        assert _cw(dev, samplerate=bad, stereo=1) == EARG
    for mode in (0, 1, 2):
        assert _ssb(dev, 8, mode=mode, bandwidth=NAN) == EARG
    assert _bank_cw(dev, 8, tone=NAN) == EARG
    assert _cw(dev, tone=NAN) == EARG
    assert _xlator(dev, 8, offset=NAN) == EARG and _xlator_real(dev, 8, offset=NAN) == EARG
    # (not finite is refused, not only NaN)
    assert _ssb(dev, 8, bandwidth=INF) == EARG and _bank_cw(dev, 8, tone=-INF) == EARG and _xlator(dev, 8, offset=INF) == EARG


def test_valid_arguments_reach_the_device_check():
    for mode in (0, 1, 2):
        for agc in (0, 1):
            assert _ssb(-1, 8, mode=mode, agc=agc) == ENODEV
    assert _ssb(-1, 8, bandwidth=0.0) == ENODEV and _ssb(-1, 8, bandwidth=-2800.0) == ENODEV
    for tone in (0.0, -800.0, 800.0):
        assert _bank_cw(-1, 8, tone=tone) == ENODEV and _cw(-1, tone=tone) == ENODEV
    assert _cw(-1, stereo=1) == ENODEV
    for offset in (0.0, -3.0, 40.0):
        assert _xlator(-1, 1, offset=offset) == ENODEV


def test_null_handles():
    assert lib.sdrgpu_bank_xlator_set_offset(None, 0.1) == EARG
    assert lib.sdrgpu_cw_set_tone(None, 700.0) == EARG
    assert lib.sdrgpu_bank_xlator_create(None, 0, 4, 0.3) == EARG
    assert lib.sdrgpu_bank_xlator_real_create(None, 0, 4, 0.3) == EARG
    assert lib.sdrgpu_bank_ssb_create(None, 0, 4, 0, 2800.0, FS, 1, ATTACK, DECAY) == EARG
    assert lib.sdrgpu_bank_cw_create(None, 0, 4, 800.0, 1, ATTACK, DECAY, FS) == EARG
    assert lib.sdrgpu_cw_create(None, 0, 800.0, 1, ATTACK, DECAY, FS, 0) == EARG


def _without_handle(cls, streams):
    """A bank object with no handle: process() checks the shape before it touches one."""
    b = cls.__new__(cls)
    b._h, b.streams, b.in_dtype, b.out_dtype = None, streams, np.complex64, np.float32
    return b


@pytest.mark.parametrize("cls", ["BankXlator", "BankSSB", "BankCW"])
def test_python_classes_refuse_a_wrong_shape(cls):
    b = _without_handle(getattr(dsp, cls), 5)
    for shape in [(7, 4), (7, 6), (35,), (7, 5, 1)]:
        with pytest.raises(ValueError):
            b.process(np.zeros(shape, np.complex64))
    with pytest.raises(sdrpp_amd.SdrGpuError):                  # the right shape passes the check (and then finds no handle)
        b.process(np.zeros((7, 5), np.complex64))
    with pytest.raises(sdrpp_amd.SdrGpuError):
        b.set_offset(0.1)
