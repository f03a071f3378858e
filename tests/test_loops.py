"""Serial loops and the AM / SSB demodulators: libsdrgpu (HIP) vs the oracle restatement of
loop/agc.h, correction/dc_blocker.h, demod/am.h, demod/ssb.h.

Bar: the AGC and the DC blocker are BIT-EXACT (the GPU runs the reference recurrence in the
reference's operation order, compiled without FMA contraction, IEEE divide and sqrt). AM is bit-exact up to its
low-pass FIR, whose fp32 accumulation is held to tests/_util.py fir_atol against the oracle's
fp64-accumulating FIR. SSB's xlator is the GPU NCO (<= 2 ulp per sample vs the oracle's long
double NCO), after which the AGC is the same recurrence; its bound is stated in the test.
"""
import numpy as np
import pytest

import oracle
import sdrpp_amd
from sdrpp_amd import dsp
from _util import EPS32, fir_atol, iq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"


def bursty(rng, n, complex_data):
    """Level steps over 60 dB, silent gaps (exact zeros) and single-sample spikes, so the
    attack/decay branches, the zero-amplitude branch and the clip look-ahead all run."""
    env = np.repeat(10.0 ** rng.uniform(-3, 0, n // 500 + 1), 500)[:n]
    x = iq(rng, n) if complex_data else rng.uniform(-1, 1, n).astype(np.float32)
    x = (x * env.astype(np.float32)).astype(x.dtype)
    x[n // 3:n // 3 + 700] = 0
    spikes = rng.integers(0, n, 12)
    x[spikes] *= 50
    return x


@pytest.mark.parametrize("complex_data", [False, True])
@pytest.mark.parametrize("blocks", [[48000], [1, 1023, 1024, 1025, 4000, 0, 37, 20000]])
def test_agc_bit_exact(complex_data, blocks, rng):
    n = sum(blocks) + 3000
    x = bursty(rng, n, complex_data)
    args = (1.0, 50.0 / 48000, 5.0 / 48000, 10e6, 10.0, float("inf"))
    g = dsp.AGC(*args, complex_data=complex_data)
    o = oracle.AGC(complex_data, *args)
    i = 0
    for b in blocks + [n - sum(blocks)]:
        yg, yo = g.process(x[i:i + b]), o.process(x[i:i + b])
        assert yg.shape == yo.shape
        assert np.array_equal(yg.view(np.uint32), yo.view(np.uint32)), f"block at {i}: max diff {np.abs(yg - yo).max()}"
        i += b
    assert g.get_gain() == o.get_gain()


@pytest.mark.parametrize("complex_data", [False, True])
def test_agc_disabled_and_set_gain(complex_data, rng):
    x = bursty(rng, 30000, complex_data)
    args = (1.0, 0.01, 0.001, 10e6, 10.0, float("inf"))
    g, o = dsp.AGC(*args, complex_data=complex_data), oracle.AGC(complex_data, *args)
    for obj in (g, o):
        obj.set_enabled(False)
        obj.set_gain(3.5)                  # AM::setAGCGain path: fixed gain, clip at maxOutputAmp
    a, b = g.process(x[:10000]), o.process(x[:10000])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for obj in (g, o):
        obj.set_enabled(True)
    a, b = g.process(x[10000:]), o.process(x[10000:])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("complex_data", [False, True])
def test_dc_blocker_bit_exact(complex_data, rng):
    n = 50000
    x = (iq(rng, n) + (0.3 + 0.2j)).astype(np.complex64) if complex_data else (rng.uniform(-1, 1, n) + 0.25).astype(np.float32)
    rate = 10.0 / 48000
    g, o = dsp.DCBlocker(rate, complex_data), oracle.DCBlocker(rate, complex_data)
    for s, e in [(0, 1), (1, 3000), (3000, 3000), (3000, 50000)]:
        a, b = g.process(x[s:e]), o.process(x[s:e])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the offset converges to the DC level (the block's purpose)
    tail = g.process(x[:20000])
    assert abs(np.mean(tail[-5000:])) < 0.02


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_am_vs_oracle(mode, rng):
    fs = 48000.0
    n = 60000
    t = np.arange(n)
    carrier = (1.0 + 0.6 * np.sin(2 * np.pi * 700 * t / fs)) * np.exp(1j * (2 * np.pi * 300 * t / fs + 0.3))
    x = (0.05 * carrier + 0.001 * iq(rng, n)).astype(np.complex64)
    x[20000:21000] *= 40                                   # a burst: clip look-ahead
    args = (mode, 10000.0, 50.0 / fs, 5.0 / fs, 10.0 / fs, fs)
    g, o = dsp.AM(*args), oracle.AM(*args, precise=True)
    lpf = oracle.low_pass(5000.0, 500.0, fs)
    for s, e in [(0, 4800), (4800, 30000), (30000, n)]:
        a, b = g.process(x[s:e]), o.process(x[s:e])
        assert a.shape == b.shape
        # the FIR input is bit-identical (AGC/|x|/DC block exact), so the only difference is
        # the LPF's fp32 vs fp64 accumulation
        pre = np.abs(b).max() if b.size else 1.0
        assert np.abs(a - b).max() <= fir_atol(lpf, np.array([pre * 2])), f"mode {mode} block {s}"


def test_am_stereo_interleave(rng):
    fs = 48000.0
    x = (0.1 * iq(rng, 20000)).astype(np.complex64)
    args = (2, 8000.0, 50.0 / fs, 5.0 / fs, 10.0 / fs, fs)
    mono = dsp.AM(*args).process(x)
    st = dsp.AM(*args, stereo=True).process(x)
    assert np.array_equal(st["l"], mono) and np.array_equal(st["r"], mono)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("agc", [True, False])
def test_ssb_vs_oracle(mode, agc, rng):
    fs = 24000.0
    n = 48000
    t = np.arange(n)
    x = (0.2 * np.exp(2j * np.pi * 1100 * t / fs) + 0.05 * np.exp(-2j * np.pi * 700 * t / fs)).astype(np.complex64)
    x = (x + 0.002 * iq(rng, n)).astype(np.complex64)
    args = (mode, 2800.0, fs, agc, 50.0 / fs, 5.0 / fs)
    g, o = dsp.SSB(*args), oracle.SSB(*args)
    for s, e in [(0, 2400), (2400, n)]:
        a, b = g.process(x[s:e]), o.process(x[s:e])
        assert a.shape == b.shape
        scale = max(np.abs(b).max(), 1e-30)
        err = np.abs(a - b)
        if agc:
            # xlator: <= ~4 ulp relative per sample (GPU NCO vs long double); the AGC
            # recurrence carries such perturbations at the output scale: bound 1e-5 of it
            assert err.max() <= 1e-5 * scale + 16 * EPS32 * scale, f"mode {mode} agc {agc} block {s}"
        else:
            # AGC disabled (ssb.h:31): fixed gain min(initGain = inf, maxGain) = 1e7 with the
            # clip at 10 -- a hard limiter, which maps an ulp-level xlator difference at a
            # near-zero sample to a 1e7-times larger one. Clipped samples (|y| = 10) must agree
            # exactly in sign and value; the rare unclipped ones are the limiter's linear region.
            clipped = np.abs(b) >= 10.0 * (1 - 1e-6)
            assert clipped.mean() > 0.99
            assert np.all(np.abs(a[clipped] - b[clipped]) <= 16 * EPS32 * 10.0), f"mode {mode} block {s}"


def fm_stereo_iq(n, fs, left_hz=1000.0, right_hz=0.0, seed=3):
    """FM broadcast: mpx = 0.45 (L+R) + 0.45 (L-R) cos(2 th) + 0.1 cos(th), th = 19 kHz pilot
    phase, 75 kHz deviation, plus a little complex noise."""
    t = np.arange(n) / fs
    L = np.sin(2 * np.pi * left_hz * t) if left_hz else np.zeros(n)
    R = np.sin(2 * np.pi * right_hz * t) if right_hz else np.zeros(n)
    th = 2 * np.pi * 19000 * t
    mpx = 0.45 * (L + R) + 0.45 * (L - R) * np.cos(2 * th) + 0.1 * np.cos(th)
    ph = 2 * np.pi * 75000 * np.cumsum(mpx) / fs
    rng = np.random.default_rng(seed)
    return (0.5 * np.exp(1j * ph) + 1e-3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


@pytest.mark.parametrize("low_pass", [True, False])
def test_broadcast_fm_stereo_vs_oracle(low_pass):
    """Stereo decoder (pilot band-pass -> PLL -> matrix -> low-pass) vs the oracle's float
    restatement of broadcast_fm.h / pll.h. The PLL uses cosf/sinf/atan2f, whose last bits
    differ between the GPU's and the host's libm: the loop filter keeps those differences at
    the ulp level of the phase, so the audio agrees to 2e-5 of full scale."""
    fs = 240000.0
    x = fm_stereo_iq(72000, fs)
    g = dsp.BroadcastFM(100000, fs, low_pass, stereo=True)
    o = oracle.BroadcastFMStereo(100000, fs, True, low_pass)
    for s, e in [(0, 7000), (7000, 40000), (40000, 72000)]:
        a, b = g.process(x[s:e]), o.process(x[s:e])
        assert a.shape == b.shape
        for ch in ("l", "r"):
            err = np.abs(a[ch].astype(np.float64) - b[ch]).max()
            assert err <= 2e-5 * max(np.abs(b[ch]).max(), 1.0), f"{ch} block {s}: {err:.3e}"


def test_broadcast_fm_stereo_mono_path_equals_wfm(rng):
    fs = 240000.0
    x = fm_stereo_iq(20000, fs)
    a = dsp.BroadcastFM(100000, fs, True, stereo=False).process(x)
    o = oracle.BroadcastFMStereo(100000, fs, False, True).process(x)
    assert np.abs(a["l"] - o["l"]).max() <= 2e-5 and np.array_equal(a["l"], a["r"])


CHUNK_CUTS = [1, 1023, 1024, 1025, 0, 2049, 37]


def _chunk_edge_cases():
    """(name, block, oracle, stream): each serial block with the oracle its own bit-exact test uses, on
    sum(CHUNK_CUTS) samples from a generator of this test's own (the session `rng` is not advanced)."""
    from _restated import NoiseBlankerRef, bursty as if_bursty
    rng = np.random.default_rng(0x10C5)
    n = sum(CHUNK_CUTS)
    rate = 10.0 / 48000
    yield ("dcb_f32", dsp.DCBlocker(rate, False), oracle.DCBlocker(rate, False),
           (rng.uniform(-1, 1, n) + 0.25).astype(np.float32))
    yield ("dcb_c64", dsp.DCBlocker(rate, True), oracle.DCBlocker(rate, True),
           (iq(rng, n) + (0.3 + 0.2j)).astype(np.complex64))
    yield ("deemp_mono", dsp.Deemphasis(50e-6, 48000, False), oracle.Deemphasis(50e-6, 48000, False),
           rng.uniform(-1, 1, n).astype(np.float32))
    st = np.zeros(n, dsp.STEREO)
    st["l"], st["r"] = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    yield ("deemp_stereo", dsp.Deemphasis(50e-6, 48000, True), oracle.Deemphasis(50e-6, 48000, True), st)
    for rate, level in [(500.0 / 24000.0, 10.0), (500.0 / 250000.0, 2.0)]:   # test_noise_blanker_bit_exact's
        yield (f"nb_{level:g}", dsp.NoiseBlanker(rate, level), NoiseBlankerRef(rate, level), if_bursty(rng, n))


def test_serial_blocks_chunk_edges():
    """The serial blocks' walk stages 1024 samples at a time: calls of 1 / 1023 / 1024 / 1025 / 0 / 2049 /
    37 samples put a call's end before, on and after a chunk edge and run two full chunks plus one sample
    in one call. Every call's output is bit-identical to the block's oracle."""
    def bits(a):
        return np.ascontiguousarray(a).view(np.uint32)

    for name, g, o, x in _chunk_edge_cases():
        i = 0
        for c in CHUNK_CUTS:
            a, b = g.process(x[i:i + c]), o.process(x[i:i + c])
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), f"{name}: call of {c} at {i}"
            i += c
        assert i == len(x)


def test_broadcast_fm_stereo_split_invariant():
    """BroadcastFM stereo with RDS, one call against the same stream in seven: l and r are bit-identical.
    The state (PLL phase / frequency, the delay line, every FIR history) is on the device, the FIR streams
    are split-invariant and the libm calls deterministic. Calls shorter than, equal to and longer than the
    delay line exercise the hist / in split of its carry; 1024 and 1025 cross a chunk edge of the PLL walk.

    The RDS samples are not bit-identical between the two cuttings (seen before this test's code was
    touched: the last bits differ, 1e-9 at a 1e-3 sample): the branch's xlator reads a per-call NCO table
    built from the call's start phase, so where a call starts moves the table's rounding. They are held to
    equal counts per stream and to the cascade bar of test_broadcast_fm_rds_branch, 5e-5 of the MPX peak."""
    fs = 240000.0
    ntaps = len(oracle.band_pass(18750.0, 19250.0, 3000.0, fs, True, complex_taps=True))   # the pilot filter
    delay = (ntaps - 1) // 2 + 1
    assert (ntaps, delay) == (305, 153)
    cuts = [1, delay - 1, delay, delay + 1, 1024, 1025, 700]
    n = sum(cuts)
    x = fm_stereo_iq(n, fs)
    one = dsp.BroadcastFM(100000, fs, True, stereo=True, rds=True)
    whole = one.process(x)
    whole_rds = one.rds_output()
    many = dsp.BroadcastFM(100000, fs, True, stereo=True, rds=True)
    audio, rds = [], []
    i = 0
    for c in cuts:
        audio.append(many.process(x[i:i + c]))
        rds.append(many.rds_output())
        i += c
    audio, rds = np.concatenate(audio), np.concatenate(rds)
    assert audio.shape == whole.shape == (n,) and rds.shape == whole_rds.shape and len(rds) > 50
    for ch in ("l", "r"):
        assert np.array_equal(audio[ch].view(np.uint32), whole[ch].view(np.uint32)), ch
    mpx_peak = np.abs(oracle.Quadrature(2 * np.pi * 100000 / fs).process(x)).max()
    err = np.abs(rds - whole_rds).max()
    print(f"rds split vs whole: max diff {err:.3e}, bar {5e-5 * mpx_peak:.3e}")
    assert err <= 5e-5 * mpx_peak
