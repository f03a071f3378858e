"""Host side of the IF noise reduction blocks (no GPU): FMIF's window against the numpy fp64
formula of window/nuttall.h + window/cosine.h (fm_if.h:112: fftWin[i] = nuttall(i, bins - 1)), and
the argument checks of sdrgpu_fmif_create, which come before the device is selected."""
import ctypes

import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import dsp

BINS = [3, 9, 15, 16, 31, 32]
NUTTALL = (0.355768, 0.487396, 0.144232, 0.012604)


def nuttall64(bins):
    n = np.arange(bins, dtype=np.float64)
    w = np.zeros(bins)
    for i, c in enumerate(NUTTALL):
        w += (-1.0) ** i * c * np.cos(i * 2.0 * np.pi * n / (bins - 1))
    return w


@pytest.mark.parametrize("bins", BINS)
def test_fmif_window(bins):
    w = dsp.fmif_window(bins)
    assert w.dtype == np.float32 and w.shape == (bins,)
    ref = nuttall64(bins)
    # 1 f32 ulp of each value, plus the fp64 formula's own uncertainty: four terms of magnitude
    # <= 0.49, each carrying a few 2^-53 relative from cos and the products, summed (< 1e-15). It only
    # matters at the two ends, where the coefficients cancel to ~-2e-17 (they sum to 0 in decimal).
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 1e-15
    assert np.all(np.abs(w.astype(np.float64) - ref) <= ulp), np.abs(w - ref).max()
    assert np.array_equal(w, w[::-1])
    assert w[0] == w[bins - 1] and abs(w[0]) < 1e-3
    assert w[bins // 2] > 0.9 and np.all(w[1:-1] > 0)


@pytest.mark.parametrize("bins", [0, 2, 33])
def test_fmif_create_checks_bins_before_the_device(bins):
    lib = sdrpp_amd.lib
    h = ctypes.c_void_p()
    bad = lib.sdrgpu_device_count()          # first index past the last device
    assert lib.sdrgpu_fmif_create(ctypes.byref(h), bad, bins) == -1   # SDRGPU_EARG
    assert b"bins" in lib.sdrgpu_last_error()
    w = np.zeros(64, np.float32)
    assert lib.sdrgpu_fmif_window(bins, w.ctypes.data_as(ctypes.c_void_p)) == -1


def test_fmif_create_without_device_reports_enodev():
    lib = sdrpp_amd.lib
    h = ctypes.c_void_p()
    bad = lib.sdrgpu_device_count()
    assert lib.sdrgpu_fmif_create(ctypes.byref(h), bad, 32) == -5     # SDRGPU_ENODEV
    assert b"not available" in lib.sdrgpu_last_error()
    assert lib.sdrgpu_noise_blanker_create(ctypes.byref(h), bad, 500.0 / 24000.0, 10.0) == -5
    assert lib.sdrgpu_squelch_create(ctypes.byref(h), bad, -50.0) == -5
