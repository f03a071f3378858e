"""The entry rule of block handles (csrc/blocks.h): only the C entry points select the device, own the
handle's stream and wait for the device; block members assume the handle's device is current.

A. A setter or a reset issued between two asynchronous calls (process_dev on a non-default stream, no
synchronise in between) gives the bits of the synchronous sequence process / setter / process on a fresh
handle of the same arguments: the entry point waits before it rewrites device state that the queued call still
reads (NCO tables, tap tables and history, the latched gain, the state a reset clears). The first call is 2^20
samples, so that it is plausibly still in flight when the setter runs; the second is 4099.

B. With two GPUs: a handle created on device 1 and called from a thread parked on device 0 (a tiny
dsp.convert(..., device=0) before every call) gives the bits of the same sequence on a device-0 handle."""
import functools

import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import dsp

pytestmark = pytest.mark.gpu

N1, N2 = 1 << 20, 4099
VFO = (61.44e6, 240e3, 200e3, 2.5e6)
AGC = (1.0, 50.0 / 48000.0, 5.0 / 48000.0, 1e6, 10.0, 1.0)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"


@functools.lru_cache(maxsize=None)
def _noise(n, seed):
    """n complex64 samples, uniform in the unit square (built once per size, only read afterwards)."""
    g = np.random.default_rng(seed)
    x = (g.uniform(-1, 1, n) + 1j * g.uniform(-1, 1, n)).astype(np.complex64)
    x.setflags(write=False)
    return x


def _lowpass(n, cutoff):
    k = np.arange(n) - (n - 1) / 2.0
    return (np.sinc(2.0 * cutoff * k) * 2.0 * cutoff * np.hanning(n + 2)[1:-1]).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b, what):
    assert a.shape == b.shape, f"{what}: {a.shape[0]} outputs, expected {b.shape[0]}"
    assert np.array_equal(_bits(a), _bits(b)), f"{what}: bits differ"


# ---- A: a setter or reset between two asynchronous calls ---------------------------------------------
def _sync(make, between, x1, x2):
    b = make()
    y1 = b.process(x1)
    between(b)
    return y1, b.process(x2)


def _async(make, between, x1, x2):
    """process_dev(x1), `between` at once, process_dev(x2) on one non-default stream, one synchronise."""
    import torch
    b = make()
    s = torch.cuda.Stream()
    xd = [torch.from_numpy(np.array(x).view(np.float32)).cuda() for x in (x1, x2)]   # (a writable copy)
    npd = np.dtype(b.out_dtype)
    yd = [torch.zeros(max(b.out_count(len(x)), 1) * npd.itemsize // 4 + 2, dtype=torch.float32, device="cuda") for x in (x1, x2)]
    torch.cuda.synchronize()
    n1 = b.process_dev(xd[0].data_ptr(), len(x1), yd[0].data_ptr(), s.cuda_stream)
    between(b)
    n2 = b.process_dev(xd[1].data_ptr(), len(x2), yd[1].data_ptr(), s.cuda_stream)
    s.synchronize()
    return tuple(y.cpu().numpy().view(npd)[:n] for y, n in zip(yd, (n1, n2)))


CASES_A = {
    "rxvfo_set_offset": (lambda: dsp.RxVFO(*VFO), lambda b: b.set_offset(-1.25e6), False),
    "fir_set_taps": (lambda: dsp.FIR(_lowpass(64, 0.05), 8), lambda b: b.set_taps(_lowpass(33, 0.04)), False),
    "rxvfo_reset": (lambda: dsp.RxVFO(*VFO), lambda b: b.reset(), True),
    "agc_set_gain": (lambda: dsp.AGC(*AGC, complex_data=True), lambda b: b.set_gain(0.25), False),
}


@pytest.mark.parametrize("case", sorted(CASES_A))
def test_setter_between_async_calls_equals_sync(case):
    make, between, repeat = CASES_A[case]
    x1 = _noise(N1, 16)
    x2 = x1 if repeat else _noise(N2, 17)
    r1, r2 = _sync(make, between, x1, x2)
    assert len(r1) > 0 and len(r2) > 0
    a1, a2 = _async(make, between, x1, x2)
    _same(a1, r1, f"{case}: first call")
    _same(a2, r2, f"{case}: call after the setter")
    if repeat:   # after a reset the handle is a fresh one
        _same(r2, r1, f"{case}: synchronous call after reset against a fresh handle")
        _same(a2, r1, f"{case}: asynchronous call after reset against a fresh handle")


# ---- B: entry points select the handle's device ------------------------------------------------------
def _park():
    """Leaves the calling thread on device 0."""
    dsp.convert(0, np.zeros(2, np.uint8), device=0)


def _seq(b, steps):
    """Runs the steps on b, the thread parked on device 0 before each; the values they return."""
    out = []
    for step in steps:
        _park()
        r = step(b)
        if r is not None:
            out.append(np.atleast_1d(np.asarray(r)))
    return out


def X():
    return _noise(4096, 18)


def P(b):
    return b.process(X())


CASES_B = {
    "rxvfo": (lambda d: dsp.RxVFO(*VFO, device=d), [P, lambda b: b.set_offset(-1.25e6), P, lambda b: b.reset(), P]),
    "fir_set_taps": (lambda d: dsp.FIR(_lowpass(64, 0.05), 8, device=d), [P, lambda b: b.set_taps(_lowpass(33, 0.04)), P]),
    "agc_gain": (lambda d: dsp.AGC(*AGC, complex_data=True, device=d),
                 [P, lambda b: b.get_gain(), lambda b: b.set_gain(0.25), lambda b: b.get_gain(), P, lambda b: b.get_gain()]),
    "squelch_is_muted": (lambda d: dsp.Squelch(-10.0, device=d),
                         [P, lambda b: b.is_muted(), lambda b: b.process(X() * np.float32(1e-3)), lambda b: b.is_muted()]),
    "fmif_set_bins": (lambda d: dsp.FMIF(32, device=d), [P, lambda b: b.set_bins(16), P]),
    "cw_set_tone": (lambda d: dsp.CW(800.0, True, 50.0 / 24000.0, 5.0 / 24000.0, 24000.0, device=d),
                    [P, lambda b: b.set_tone(650.0), P]),
    "broadcast_fm_rds": (lambda d: dsp.BroadcastFM(75e3, 240e3, device=d, stereo=True),
                         [lambda b: b.set_rds(True), lambda b: b.process(_noise(24000, 19)).view(np.float32),
                          lambda b: b.rds_output()]),
}


@pytest.mark.parametrize("case", sorted(CASES_B))
def test_entry_points_select_the_handles_device(case):
    if sdrpp_amd.lib.sdrgpu_device_count() < 2:
        pytest.skip("needs at least 2 visible GPUs")
    make, steps = CASES_B[case]
    _park()
    got = _seq(make(1), steps)
    ref = _seq(make(0), steps)
    assert len(got) == len(ref) >= 2
    if case == "broadcast_fm_rds":
        assert len(ref[-1]) > 0, "the RDS branch gave no output"
    for k, (a, r) in enumerate(zip(got, ref)):
        _same(a, r, f"{case}: value {k}")
