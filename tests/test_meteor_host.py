"""The Meteor demodulator and the carrier loops, the host side (no GPU): every new create function checks all its
arguments before it selects the device, so the refusals (SDRGPU_EARG) show on a machine without one, and valid
arguments there report the missing device. The setters refuse a handle that holds no such block."""
import ctypes

import numpy as np
import pytest

from sdrpp_amd import lib

EARG, ENODEV = -1, -5
PI32 = float(np.float32(3.1415926535))
NAN, INF = float("nan"), float("inf")


def _create(fn, *args):
    h = ctypes.c_void_p()
    return fn(ctypes.byref(h), *args)


# name -> create(device, streams (None: the single-stream block), **changes): valid arguments unless a keyword changes one
def _loop(single, bank, extra=()):
    def create(dev, streams=None, bandwidth=0.01, phase=0.0, freq=0.0, limits=(-PI32, PI32)):
        head = (dev,) if streams is None else (dev, streams)
        return _create(single if streams is None else bank, *head, bandwidth, *extra, phase, freq, *limits)
    return create


def _meteor(dev, streams=None, rates=(72000.0, 150000.0), rrc=33, bandwidth=0.005, mu_gain=0.01, rel=0.01, agc=0.1):
    head = (dev,) if streams is None else (dev, streams)
    fn = lib.sdrgpu_meteor_create if streams is None else lib.sdrgpu_bank_meteor_create
    return _create(fn, *head, *rates, rrc, 0.6, agc, bandwidth, 0, 1, 1e-6, mu_gain, rel)


LOOPS = {
    "pll": _loop(lib.sdrgpu_pll_create, lib.sdrgpu_bank_pll_create),
    "carrier_pll": _loop(lib.sdrgpu_carrier_pll_create, lib.sdrgpu_bank_carrier_pll_create),
    "meteor_costas": _loop(lib.sdrgpu_meteor_costas_create, lib.sdrgpu_bank_meteor_costas_create, extra=(1,)),
}
CREATES = dict(LOOPS, meteor=_meteor)


@pytest.mark.parametrize("streams", [None, 65])
@pytest.mark.parametrize("name", sorted(CREATES))
def test_create_without_device(name, streams):
    assert CREATES[name](-1, streams) == ENODEV
    assert b"not available" in lib.sdrgpu_last_error()


@pytest.mark.parametrize("streams", [0, -1, -64])
@pytest.mark.parametrize("name", sorted(CREATES))
def test_streams_below_one_are_refused(name, streams):
    assert CREATES[name](-1, streams) == EARG
    assert CREATES[name](0, streams) == EARG


@pytest.mark.parametrize("dev", [-1, 0])
@pytest.mark.parametrize("streams", [None, 8])
@pytest.mark.parametrize("name", sorted(LOOPS))
def test_loop_argument_checks_need_no_device(name, streams, dev):
    make = LOOPS[name]
    assert make(dev, streams, limits=(1.0, 1.0)) == EARG         # assert(maxFreq > minFreq)
    assert make(dev, streams, limits=(0.5, -0.5)) == EARG
    assert make(dev, streams, limits=(-PI32, INF)) == EARG
    assert make(dev, streams, limits=(-2000.0, PI32)) == EARG    # beyond 1024 rad
    assert make(dev, streams, bandwidth=NAN) == EARG
    assert make(dev, streams, phase=INF) == EARG
    assert make(dev, streams, phase=1025.0) == EARG
    assert make(dev, streams, freq=NAN) == EARG
    assert make(dev, streams, freq=-1025.0) == EARG


@pytest.mark.parametrize("dev", [-1, 0])
@pytest.mark.parametrize("streams", [None, 8])
def test_meteor_argument_checks_need_no_device(streams, dev):
    assert _meteor(dev, streams, rates=(0.0, 150000.0)) == EARG  # symbol and sample rates
    assert _meteor(dev, streams, rates=(72000.0, -1.0)) == EARG
    assert _meteor(dev, streams, rates=(NAN, 150000.0)) == EARG
    assert _meteor(dev, streams, rrc=0) == EARG                  # tap counts
    assert _meteor(dev, streams, rrc=-3) == EARG
    assert _meteor(dev, streams, bandwidth=NAN) == EARG
    assert _meteor(dev, streams, mu_gain=3.0) == EARG            # MM: omega (1 - rel) - muGain < 1
    assert _meteor(dev, streams, rates=(150000.0, 150000.0)) == EARG   # omega = 1
    assert _meteor(dev, streams, rel=0.0) == EARG
    assert _meteor(dev, streams, mu_gain=NAN) == EARG


def test_null_handles_and_setters():
    assert lib.sdrgpu_pll_create(None, 0, 0.01, 0.0, 0.0, -PI32, PI32) == EARG
    assert lib.sdrgpu_carrier_pll_create(None, 0, 0.01, 0.0, 0.0, -PI32, PI32) == EARG
    assert lib.sdrgpu_meteor_costas_create(None, 0, 0.005, 1, 0.0, 0.0, -PI32, PI32) == EARG
    assert lib.sdrgpu_meteor_create(None, 0, 72000.0, 150000.0, 33, 0.6, 0.1, 0.005, 0, 0, 1e-6, 0.01, 0.01) == EARG
    assert lib.sdrgpu_bank_pll_create(None, 0, 4, 0.01, 0.0, 0.0, -PI32, PI32) == EARG
    assert lib.sdrgpu_bank_carrier_pll_create(None, 0, 4, 0.01, 0.0, 0.0, -PI32, PI32) == EARG
    assert lib.sdrgpu_bank_meteor_costas_create(None, 0, 4, 0.005, 1, 0.0, 0.0, -PI32, PI32) == EARG
    assert lib.sdrgpu_bank_meteor_create(None, 0, 4, 72000.0, 150000.0, 33, 0.6, 0.1, 0.005, 0, 0, 1e-6, 0.01, 0.01) == EARG
    # the setters on no handle: refused, and no device is touched
    assert lib.sdrgpu_meteor_costas_set_broken_modulation(None, 1) == EARG
    assert lib.sdrgpu_meteor_set_broken_modulation(None, 1) == EARG
    assert lib.sdrgpu_meteor_set_oqpsk(None, 1) == EARG
