"""Inputs and measures of the broadcast-FM bank tests (tests/test_bank_wfm.py), numpy only.

Stream k is a stereo FM broadcast built as tests/test_loops.py fm_stereo_iq builds its signal, with its own
tones, phases, amplitude and noise, so that no two columns agree and a swapped column fails:
  L = sin(2 pi (700 + 40 k) t + 0.3 k),  R = 0.6 sin(2 pi (1900 + 55 k) t + 0.1 k),  pilot phase 0.37 k
  mpx = 0.45 (L + R) + 0.45 (L - R) cos(2 th) + 0.1 cos(th),  th = 2 pi 19000 t + 0.37 k
  x = (0.3 + 0.1 (k mod 5)) exp(j (2 pi 75000 cumsum(mpx) / fs + 0.2 k)) + 1e-3 complex noise of default_rng(500 + k)
"""
import numpy as np

FS = 240000.0
DEVIATION = 100000.0
TX_DEVIATION = 75000.0
FRAMES = 4200
SETTLED = slice(2200, 4200)                                     # rows past the filters' and the PLL's transients


def l_tone(k):
    return 700.0 + 40.0 * k


def r_tone(k):
    return 1900.0 + 55.0 * k


def stereo_stream(k, n=FRAMES, fs=FS):
    t = np.arange(n) / fs
    L = np.sin(2 * np.pi * l_tone(k) * t + 0.3 * k)
    R = 0.6 * np.sin(2 * np.pi * r_tone(k) * t + 0.1 * k)
    th = 2 * np.pi * 19000 * t + 0.37 * k
    mpx = 0.45 * (L + R) + 0.45 * (L - R) * np.cos(2 * th) + 0.1 * np.cos(th)
    ph = 2 * np.pi * TX_DEVIATION * np.cumsum(mpx) / fs + 0.2 * k
    rng = np.random.default_rng(500 + k)
    amp = 0.3 + 0.1 * (k % 5)
    return (amp * np.exp(1j * ph) + 1e-3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def stereo_bank(S, n=FRAMES, fs=FS):
    """(n, S) complex64: column k is stereo_stream(k)"""
    return np.ascontiguousarray(np.stack([stereo_stream(k, n, fs) for k in range(S)], axis=1))


def tone_amplitude(y, hz, rows=SETTLED, fs=FS):
    """the amplitude of the tone at `hz` in y[rows]: the length of its projection onto exp(j 2 pi hz t)"""
    y = np.asarray(y, np.float64)[rows]
    t = np.arange(rows.start, rows.stop) / fs
    return 2.0 * abs(np.mean(y * np.exp(-2j * np.pi * hz * t)))
