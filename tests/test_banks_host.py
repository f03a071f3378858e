"""Stream banks, the host side (no GPU): every create function checks all its arguments before it
selects the device, so the refusals (SDRGPU_EARG) show on a machine without one, and valid arguments
there report the missing device."""
import ctypes

import numpy as np
import pytest

from sdrpp_amd import lib, F32, C64

EARG, ENODEV = -1, -5
PI32 = float(np.float32(3.1415926535))
TAPS = np.linspace(0.1, 0.8, 8).astype(np.float32)
TP = TAPS.ctypes.data_as(ctypes.c_void_p)


def _create(fn, *args):
    h = ctypes.c_void_p()
    return fn(ctypes.byref(h), *args)


# name -> create(device, streams, **changes): valid arguments unless a keyword changes one
def _quadrature(dev, streams):
    return _create(lib.sdrgpu_bank_quadrature_create, dev, streams, 0.4)


def _fir(dev, streams, dtype=C64, ntaps=8):
    return _create(lib.sdrgpu_bank_fir_create, dev, streams, dtype, TP, ntaps)


def _fast_agc(dev, streams, dtype=C64):
    return _create(lib.sdrgpu_bank_fast_agc_create, dev, streams, dtype, 1.0, 1e6, 0.1, 1.0)


def _costas(dev, streams, order=2, limits=(-PI32, PI32)):
    return _create(lib.sdrgpu_bank_costas_create, dev, streams, order, 0.005, 0.0, 0.0, *limits)


def _mm(dev, streams, dtype=F32, omega=4.0, mu_gain=0.01, bank=(128, 8)):
    return _create(lib.sdrgpu_bank_mm_create, dev, streams, dtype, omega, 2.5e-5, mu_gain, 0.01, *bank)


def _psk(dev, streams, order=4, rrc=31, mu_gain=0.01, rates=(1.0, 4.0)):
    return _create(lib.sdrgpu_bank_psk_create, dev, streams, order, *rates, rrc, 0.6, 0.01, 0.005, 2.5e-5, mu_gain, 0.01)


def _gfsk(dev, streams, rrc=31, mu_gain=0.01, rates=(12000.0, 48000.0)):
    return _create(lib.sdrgpu_bank_gfsk_create, dev, streams, *rates, 3000.0, rrc, 0.6, 2.5e-5, mu_gain, 0.01)


CREATES = {"quadrature": _quadrature, "fir": _fir, "fast_agc": _fast_agc, "costas": _costas, "mm": _mm, "psk": _psk,
           "gfsk": _gfsk}


@pytest.mark.parametrize("name", sorted(CREATES))
def test_create_without_device(name):
    assert CREATES[name](-1, 65) == ENODEV
    assert b"not available" in lib.sdrgpu_last_error()


@pytest.mark.parametrize("streams", [0, -1, -64])
@pytest.mark.parametrize("name", sorted(CREATES))
def test_streams_below_one_are_refused(name, streams):
    assert CREATES[name](-1, streams) == EARG
    assert CREATES[name](0, streams) == EARG


@pytest.mark.parametrize("dev", [-1, 0])
def test_argument_checks_need_no_device(dev):
    # a Costas order of 3 (static_assert(ORDER ...)), alone and inside PSK; minFreq >= maxFreq
    assert _costas(dev, 8, order=3) == EARG
    assert _psk(dev, 8, order=3) == EARG
    assert _costas(dev, 8, limits=(1.0, 1.0)) == EARG
    # MM: omega (1 - rel) - muGain < 1, alone and at the end of PSK / GFSK
    assert _mm(dev, 8, omega=1.0) == EARG                       # 0.99 - 0.01
    assert _mm(dev, 8, dtype=C64, omega=1.02) == EARG           # 1.0098 - 0.01
    assert _mm(dev, 8, mu_gain=3.0) == EARG                     # 3.96 - 3
    assert _psk(dev, 8, mu_gain=3.0) == EARG
    assert _gfsk(dev, 8, mu_gain=3.0) == EARG
    assert _psk(dev, 8, rates=(4.0, 4.0)) == EARG               # omega = 1
    # MM: interpolator bank outside [1, 1024] x [1, 64]
    for bank in [(0, 8), (1025, 8), (128, 0), (128, 65)]:
        assert _mm(dev, 8, bank=bank) == EARG, bank
    # ntaps = 0: the FIR bank, and the RRC of PSK / GFSK
    assert _fir(dev, 8, ntaps=0) == EARG
    assert _fir(dev, 8, dtype=F32, ntaps=-3) == EARG
    assert _psk(dev, 8, rrc=0) == EARG
    assert _gfsk(dev, 8, rrc=0) == EARG
    assert _create(lib.sdrgpu_bank_fir_create, dev, 8, C64, None, 8) == EARG
    # element types
    assert _fir(dev, 8, dtype=2) == EARG
    assert _fast_agc(dev, 8, dtype=2) == EARG
    assert _mm(dev, 8, dtype=7) == EARG
    # symbol and sample rates
    assert _psk(dev, 8, rates=(0.0, 4.0)) == EARG
    assert _gfsk(dev, 8, rates=(12000.0, -1.0)) == EARG


def test_null_handles():
    assert lib.sdrgpu_bank_streams(None) == EARG
    assert lib.sdrgpu_bank_process(None, None, 0, None) == EARG
    assert lib.sdrgpu_bank_process_dev(None, None, 0, None, None) == EARG
    assert lib.sdrgpu_bank_out_rows(None, 4) == EARG
    assert lib.sdrgpu_bank_reset(None) == EARG
    assert lib.sdrgpu_bank_destroy(None) == 0
    assert lib.sdrgpu_bank_quadrature_create(None, 0, 4, 0.4) == EARG
