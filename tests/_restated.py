"""Numpy float32 restatements of the reference's stateful blocks, and the seeded signals their tests
use (a plain helper module: importable without a GPU).

One scalar operation per reference operation, in the reference's order, file:line cited. The device
tests (test_symsync.py, test_ifnr.py, test_banks.py, test_loops.py) hold the kernels to these
functions; tests/test_ref_blocks.py holds these functions to the reference's OWN headers, compiled by
oracle/ref_blocks.cpp and recorded in tests/golden/ref_blocks_*.npz. The per-sample loops carry a
leading batch axis (one independent stream per row).
"""
import numpy as np

from sdrpp_amd import dsp
from _util import EPS32, iq

f32 = np.float32
N = 12000
CUTS = [1, 6, 7, 8, 0, 1023, 1024, 1025, 4097]
CUTS = CUTS + [N - sum(CUTS)]
FL_M_PI = f32(3.1415926535)                                     # math/constants.h:4


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------- symbol recovery
def step(x):                                                    # math/step.h:5-17
    return np.where(x > f32(0), f32(1), f32(-1)).astype(f32)


def ref_fast_agc(xr, xi, set_point, max_gain, rate, gain):
    """fast_agc.h:60-79; xi None for float. Returns (out re, out im, final gain)."""
    set_point, max_gain, rate = f32(set_point), f32(max_gain), f32(rate)
    gain = np.full(xr.shape[0], gain, f32)
    yr, yi = np.empty_like(xr), (None if xi is None else np.empty_like(xi))
    for i in range(xr.shape[1]):
        yr[:, i] = xr[:, i] * gain                              # :63 (types.h:7 per component)
        if xi is None:
            amp = np.abs(yr[:, i])                              # :68
        else:
            yi[:, i] = xi[:, i] * gain
            amp = np.sqrt((yr[:, i] * yr[:, i]) + (yi[:, i] * yi[:, i]))   # :71, types.h:79
        gain = gain + (set_point - amp) * rate                  # :75
        gain = np.where(gain > max_gain, max_gain, gain)        # :76
    return yr, yi, gain


def critically_damped(bandwidth):
    """phase_control_loop.h:31-36 with T = float, as pll.h:20-22 calls it."""
    bw = f32(bandwidth)
    df = f32(np.sqrt(2.0) / 2.0)
    den = f32((1.0 + 2.0 * float(df) * float(bw)) + float(bw * bw))
    return (f32(4) * df * bw) / den, (f32(4) * bw * bw) / den


def trig32(p):
    return np.cos(p), np.sin(p)


def trig64(p):
    q = p.astype(np.float64)
    return np.cos(q).astype(f32), np.sin(q).astype(f32)


def ref_costas(xr, xi, order, bandwidth, init_phase=0.0, init_freq=0.0, min_freq=-FL_M_PI, max_freq=FL_M_PI, trig=trig32):
    """costas.h:17-45 over phase_control_loop.h:58-85."""
    alpha, beta = critically_damped(bandwidth)
    min_freq, max_freq = f32(min_freq), f32(max_freq)
    B, n = xr.shape
    phase, freq = np.full(B, init_phase, f32), np.full(B, init_freq, f32)
    delta = FL_M_PI - (-FL_M_PI)                                # :28
    K = f32(float(np.sqrt(f32(2.0))) - 1.0)                     # costas.h:36
    yr, yi = np.empty_like(xr), np.empty_like(xi)
    for i in range(n):
        c, s = trig(-phase)                                     # math/phasor.h:6-9
        re = (xr[:, i] * c) - (xi[:, i] * s)                    # types.h:23-25
        im = (xi[:, i] * c) + (xr[:, i] * s)
        yr[:, i], yi[:, i] = re, im
        if order == 2:
            err = re * im                                       # :29
        elif order == 4:
            err = (step(re) * im) - (step(im) * re)             # :32
        else:
            a = (step(re) * im) - (step(im) * re * K)           # :38
            b = (step(re) * im * K) - (step(im) * re)           # :41
            err = np.where(np.abs(re) >= np.abs(im), a, b)
        err = np.where(err < f32(-1), f32(-1), np.where(f32(1) < err, f32(1), err)).astype(f32)   # :44
        freq = freq + beta * err                                # pcl :60
        freq = np.where(freq > max_freq, max_freq, np.where(freq < min_freq, min_freq, freq))   # :78-79
        phase = phase + (freq + (alpha * err))                  # :64
        while np.any(phase > FL_M_PI):                          # :83-84
            phase = np.where(phase > FL_M_PI, phase - delta, phase)
        while np.any(phase < -FL_M_PI):
            phase = np.where(phase < -FL_M_PI, phase + delta, phase)
    return yr, yi


class RefMM:
    """clock_recovery/mm.h:24-156 for one stream; the work buffer's history starts as zeros."""

    def __init__(self, omega, omega_gain, mu_gain, rel, P=128, T=8, cplx=False):
        self.P, self.T, self.cplx = P, T, cplx
        self.bank = dsp.mm_interp_bank(P, T)                    # (tests/test_ref_blocks.py holds it to mm.h:173-178)
        self.alpha, self.beta, self.rel = f32(mu_gain), f32(omega_gain), rel       # :32 pcl.init(_muGain, _omegaGain, ...)
        self.hr, self.hi = np.zeros(T - 1, f32), np.zeros(T - 1, f32)
        self.trace = None                                       # a list: gets phase * P of every output, before the floor
        self.set_limits(omega)
        self.reset()

    def set_limits(self, omega):
        self.omega = omega
        self.min_freq, self.max_freq = f32(omega * (1.0 - self.rel)), f32(omega * (1.0 + self.rel))

    def clamp_freq(self):                                       # phase_control_loop.h:77-80
        if self.freq > self.max_freq:
            self.freq = self.max_freq
        elif self.freq < self.min_freq:
            self.freq = self.min_freq

    def reset(self):                                            # :87-98 (not the history)
        self.offset, self.phase, self.freq = 0, f32(0), f32(self.omega)
        self.last = f32(0)
        self.p = [(f32(0), f32(0))] * 3
        self.c = [(f32(0), f32(0))] * 3

    def set_omega(self, omega):                                 # :40-50
        self.offset, self.phase, self.freq = 0, f32(0), f32(omega)
        self.set_limits(omega)
        self.clamp_freq()

    def process(self, x):
        count, T = len(x), self.T
        x = np.asarray(x)
        br = np.concatenate([self.hr, x.real.astype(f32)])      # :102
        bi = np.concatenate([self.hi, x.imag.astype(f32)]) if self.cplx else None
        out = []
        while self.offset < count:                              # :106
            u = self.phase * f32(self.P)
            if self.trace is not None:
                self.trace.append(u)
            ph = int(np.floor(u))                               # :111
            ph = min(max(ph, 0), self.P - 1)
            taps, o = self.bank[ph], self.offset
            if not self.cplx:
                acc = f32(0)                                    # :113 volk_32f_x2_dot_prod_32f_generic
                for k in range(T):
                    acc = acc + br[o + k] * taps[k]
                out.append(acc)
                sl, so = (f32(1) if self.last > 0 else f32(-1)), (f32(1) if acc > 0 else f32(-1))
                error = (sl * acc) - (self.last * so)           # :122
                self.last = acc
            else:
                ar, ai = f32(0), f32(0)                         # :116 volk_32fc_32f_dot_prod_32fc_generic
                for k in range(T):
                    ar = ar + br[o + k] * taps[k]
                    ai = ai + bi[o + k] * taps[k]
                out.append(complex(ar, ai))
                self.p = [(ar, ai), self.p[0], self.p[1]]       # :127-133
                self.c = [(f32(1) if ar > 0 else f32(-1), f32(1) if ai > 0 else f32(-1)), self.c[0], self.c[1]]   # :134
                (p0r, p0i), (p1r, p1i), (p2r, p2i) = self.p
                (c0r, c0i), (c1r, c1i), (c2r, c2i) = self.c
                dr, di = p0r - p2r, p0i - p2i                   # :137
                er, ei = c0r - c2r, c0i - c2i
                a = (dr * c1r) - (di * (-c1i))
                b = (er * p1r) - (ei * (-p1i))
                error = a - b
            if error > f32(1):                                  # :141-142
                error = f32(1)
            if error < f32(-1):
                error = f32(-1)
            self.freq = self.freq + self.beta * error           # pcl :60
            self.clamp_freq()
            self.phase = self.phase + (self.freq + (self.alpha * error))   # :64 (CLAMP_PHASE false)
            delta = np.floor(self.phase)                        # :146
            self.offset = int(f32(self.offset) + delta)         # :147 int += float
            self.phase = self.phase - delta                     # :148
        self.offset -= count                                    # :150
        self.hr = br[count:count + T - 1].copy()                # :153
        if self.cplx:
            self.hi = bi[count:count + T - 1].copy()
        return np.array(out, np.complex64 if self.cplx else f32)


def ref_fir(x, taps):
    """filter/fir.h:62-83: out[i] = sum_k buffer[i + k] taps[k] over [T - 1 zeros || x] -- a correlation, so
    complex band-pass taps e^{-j w n} pass +w. In fp64, rounded once (the known answers do not need the
    last bit; the device FIR has its own parity tests)."""
    wide = np.complex128 if np.iscomplexobj(x) or np.iscomplexobj(taps) else np.float64
    y = np.convolve(np.asarray(x).astype(wide), np.asarray(taps).astype(wide)[::-1])[:len(x)]
    return y.astype(np.complex64 if wide is np.complex128 else f32)


def ref_fir32(x, taps, lanes=1):
    """filter/fir.h:62-83 in fp32, unfused: the dot product accumulated in ascending tap order (lanes = 1, VOLK's
    generic kernel) or in `lanes` interleaved partial sums combined at the end as (s0 + s1) + (s2 + s3)."""
    x, taps = np.asarray(x), np.asarray(taps)
    T, n = len(taps), len(x)
    buf = np.concatenate([np.zeros(T - 1, x.dtype), x])
    cx, ct = np.iscomplexobj(x), np.iscomplexobj(taps)
    re, im = [np.zeros(n, f32) for _ in range(lanes)], [np.zeros(n, f32) for _ in range(lanes)]
    for k in range(T):
        seg, j = buf[k:k + n], k % lanes
        if ct:                                                  # complex taps: (a b).re = a.re b.re - a.im b.im
            re[j] = re[j] + ((seg.real * taps[k].real) - (seg.imag * taps[k].imag))
            im[j] = im[j] + ((seg.real * taps[k].imag) + (seg.imag * taps[k].real))
        else:
            re[j] = re[j] + seg.real * taps[k]
            if cx:
                im[j] = im[j] + seg.imag * taps[k]
    sr, si = (((re[0] + re[1]) + (re[2] + re[3])), ((im[0] + im[1]) + (im[2] + im[3]))) if lanes == 4 else (re[0], im[0])
    return (sr + 1j * si).astype(np.complex64) if cx or ct else sr


def ref_slicer(x):                                              # binary_slicer.h:12-18
    return (x > f32(0)).astype(np.uint8)


def ref_diff(x, modulus, last=0):                               # differential_decoder.h:41-47
    prev = np.concatenate([[last], x[:-1]]).astype(np.int64)
    d = x.astype(np.int64) - prev + modulus
    return (np.sign(d) * (np.abs(d) % modulus)).astype(np.uint8)   # C's % truncates


# ------------------------------------------------------------------ signals
def rrc64(count, beta, Ts):
    return dsp.root_raised_cosine(count, beta, Ts).astype(np.float64)


def shaped_psk(seed, order, nsym=3000, sps=4, amp=1.0, cfo=2e-4, phase=0.3, snr_db=25.0):
    """order-PSK symbols at pi/order + q 2 pi/order, RRC(31, 0.6) shaped at `sps` samples per symbol,
    rms amplitude `amp`, carrier offset `cfo` cycles/sample. Returns (x complex64, q)."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, order, nsym)
    sym = np.exp(1j * ((np.pi / order if order > 2 else 0.0) + q * 2 * np.pi / order))
    up = np.zeros(nsym * sps, np.complex128)
    up[::sps] = sym
    s = np.convolve(up, rrc64(31, 0.6, sps))[:nsym * sps]
    s *= amp / np.sqrt(np.mean(np.abs(s[200:]) ** 2))           # rms amplitude `amp`
    n = np.arange(len(s))
    s = s * np.exp(1j * (2 * np.pi * cfo * n + phase))
    sigma = np.sqrt(np.mean(np.abs(s) ** 2) / 10 ** (snr_db / 10) / 2)
    s = s + sigma * (rng.standard_normal(len(s)) + 1j * rng.standard_normal(len(s)))
    return s.astype(np.complex64), q


def noise(seed, cplx):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, N).astype(f32)
    return (x + 1j * rng.uniform(-1, 1, N).astype(f32)).astype(np.complex64) if cplx else x


def parts(x):
    x = np.atleast_2d(x)
    return np.ascontiguousarray(x.real, f32), np.ascontiguousarray(x.imag, f32)


def mm_input(kind, cplx):
    if kind == "noise":
        return noise(77, cplx)
    x = shaped_psk(21, 4 if cplx else 2, cfo=0.0, phase=0.0 if not cplx else 0.3)[0]
    return x if cplx else np.ascontiguousarray(x.real)


SEEDS = range(8)
W_RDS = 2.0 * 3.14159265358979323846 * ((2375.0 / 2.0) / 5000.0)   # wfm.h:63
COSTAS_CASES = {
    "order2": dict(order=2, bandwidth=0.005, kw={}),
    "order4": dict(order=4, bandwidth=0.005, kw={}),
    "order8": dict(order=8, bandwidth=0.005, kw={}),
    # wfm.h:64 costas2.init(&fir.out, 0.01, 0.0, w, 0.9 w, 1.1 w) on BPSK sitting at +w
    "rds_second_loop": dict(order=2, bandwidth=0.01, shift=W_RDS,
                            kw=dict(init_phase=0.0, init_freq=W_RDS, min_freq=W_RDS - (W_RDS * 0.1), max_freq=W_RDS + (W_RDS * 0.1))),
}


def costas_input(case, seed):
    c = COSTAS_CASES[case]
    x = shaped_psk(100 + seed, c["order"])[0]
    if "shift" in c:
        x = (x * np.exp(1j * c["shift"] * np.arange(len(x)))).astype(np.complex64)
    return x


def costas_ref_and_S(case):
    """The fp64-trig restatement of seed 0's stream and S over the 8 seeds (test_symsync.py's bar)."""
    c = COSTAS_CASES[case]
    xs = np.stack([costas_input(case, s) for s in SEEDS])
    xr, xi = parts(xs)
    a = ref_costas(xr, xi, c["order"], c["bandwidth"], trig=trig32, **c["kw"])
    b = ref_costas(xr, xi, c["order"], c["bandwidth"], trig=trig64, **c["kw"])
    S = float(max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()))
    return dict(x=xs[0], ref=(b[0][0] + 1j * b[1][0]).astype(np.complex64), S=S)


def gfsk_signal(seed=41, nsym=3000, sps=4, dev_rad=2 * np.pi / 16, snr_db=25.0):
    """2-level symbols, RRC(31, 0.6) shaped, through Quadrature's inverse (cumulative phase)."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 2, nsym)
    up = np.zeros(nsym * sps)
    up[::sps] = 2.0 * b - 1.0
    h = rrc64(31, 0.6, sps)
    m = np.convolve(up, h)[:nsym * sps]
    m /= np.abs(m).max()                                        # the deviation peaks at dev_rad
    x = np.exp(1j * np.cumsum(dev_rad * m))
    sigma = np.sqrt(1.0 / 10 ** (snr_db / 10) / 2)
    x = x + sigma * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))
    return x.astype(np.complex64), b


GFSK_ARGS = (12000.0, 48000.0, 3000.0, 31, 0.6, 2.5e-5, 0.01, 0.01)   # 4 samples per symbol, deviation 2 pi / 16 rad
PSK_ARGS = (1.0, 4.0, 31, 0.6, 0.01, 0.005, 2.5e-5, 0.01, 0.01)       # after the order: 4 samples per symbol


def rds_signal(f0, snr_db, seed):
    """fs 5000: x = 0.01 (2 d[k] - 1) sin(2 pi 1187.5 t) e^{j (2 pi f0 t + 0.7)}, k = floor(1187.5 t),
    d = cumsum(b) mod 2, complex Gaussian noise at snr_db."""
    rng = np.random.default_rng(seed)
    t = np.arange(N) / 5000.0
    k = np.floor(1187.5 * t).astype(int)
    b = rng.integers(0, 2, k.max() + 1)
    d = np.cumsum(b) % 2
    s = 0.01 * (2.0 * d[k] - 1.0) * np.sin(2 * np.pi * 1187.5 * t) * np.exp(1j * (2 * np.pi * f0 * t + 0.7))
    sigma = np.sqrt(np.mean(np.abs(s) ** 2) / 10 ** (snr_db / 10) / 2)
    x = s + sigma * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    return x.astype(np.complex64), b


RDS_CASES = [(2.0, 30.0, 51), (-5.0, 20.0, 52)]


def errors_at_best_lag(got, want, lags, lo, hi):
    """(errors, lag) of got[lag + lo : lag + hi] against want[lo:hi], the best lag."""
    best = (10 ** 9, -1)
    for lag in lags:
        g = got[lag + lo:lag + hi]
        if len(g) == hi - lo:
            best = min(best, (int(np.count_nonzero(g != want[lo:hi])), lag))
    return best


def quadrant(z):
    return (np.floor(np.angle(z) / (np.pi / 2)).astype(int)) % 4


def ref_rds_chain(x):
    xr, xi = parts(x)
    yr, yi, _ = ref_fast_agc(xr, xi, 1.0, 1e6, 0.1, f32(1.0))                     # wfm.h:57
    yr, yi = ref_costas(yr, yi, 2, f32(0.005))                                     # :58
    taps = dsp.band_pass(0, 2375, 100, 5000, complex_taps=True)                   # :60
    assert len(taps) == 190
    f = ref_fir((yr[0] + 1j * yi[0]).astype(np.complex64), taps)                   # :61
    w = W_RDS
    fr, fi = parts(f)
    cr, _ = ref_costas(fr, fi, 2, 0.01, 0.0, w, w - (w * 0.1), w + (w * 0.1))      # :63-64
    soft = RefMM(5000.0 / (2375.0 / 2.0), 1e-6, 0.01, 0.01).process(cr[0])        # :66-67
    return ref_diff(ref_slicer(soft), 2), soft                                    # :68-69


# ------------------------------------------------------------------ FMIF
N_FMIF = 12000


def fmif_cuts(B, n=N_FMIF):
    cuts = [1, B - 2, B - 1, B, 0, 1023, 1024, 1025, 4097]
    while sum(cuts) > n:
        cuts.pop()
    return cuts + [n - sum(cuts)]


def fm_two_tone(rng, n):
    """Two-tone FM at 75 kHz deviation, fs = 250 kHz, -20 dB Gaussian noise, 200 exact zeros."""
    fs = 250e3
    t = np.arange(n) / fs
    m = 0.5 * np.sin(2 * np.pi * 1000.0 * t) + 0.5 * np.sin(2 * np.pi * 3000.0 * t)
    x = np.exp(1j * 2 * np.pi * 75e3 * np.cumsum(m) / fs)
    x = x + 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    x = x.astype(np.complex64)
    x[n // 2:n // 2 + 200] = 0
    return x


def fmif_inputs(kind, seed=20240607, n=N_FMIF):
    rng = np.random.default_rng(seed)   # local: the preconditions below do not depend on test order
    return fm_two_tone(rng, n) if kind == "fm" else iq(rng, n)


def fmif_spectra(x, B, hist=None):
    """X_i[k] of fm_if.h:52-55 in fp64: [i, k] over the stream with B - 1 zeros (or hist) in front."""
    w = dsp.fmif_window(B).astype(np.float64)
    h = np.zeros(B - 1, np.complex128) if hist is None else np.asarray(hist, np.complex128)
    buf = np.concatenate([h, np.asarray(x).astype(np.complex128)])
    win = np.lib.stride_tricks.sliding_window_view(buf, B)
    return np.fft.fft(win * w, axis=1), np.all(win == 0, axis=1)


def fmif_atol(B, x):
    w = dsp.fmif_window(B)
    return 8 * EPS32 * np.sqrt(B) * np.abs(w.astype(np.float64)).sum() * np.abs(x).max()


def fmif_check(out, x, B, what):
    """The FMIF bar (test_ifnr.py's module docstring); returns the undecidable share."""
    X, allzero = fmif_spectra(x, B)
    n = len(x)
    assert out.shape == (n,)
    atol = fmif_atol(B, x)
    k = np.arange(B)
    vals = X * np.exp(2j * np.pi * k * (B // 2) / B)       # every bin's value at sample B/2 of the back transform
    mag = np.abs(X)
    idx = np.argmax(mag, axis=1)                             # first maximum = lowest k
    top = np.sort(mag, axis=1)
    decidable = (top[:, -1] - top[:, -2]) >= 2 * atol
    ref = vals[np.arange(n), idx]
    ref[allzero] = 0
    err = np.abs(out.astype(np.complex128) - ref)
    # Also strict: samples whose near-maximum bins all carry the SAME output value (apart by less
    # than fp32 resolution), so no tie-break can show. At B = 3 that is every sample: nuttall(n, 2)
    # is (0, 1, 0), all three bins have magnitude |x[i-1]| and value x[i-1], and without this the
    # reference alone would count as 100 % undecidable.
    near = mag >= (top[:, -1] - 2 * atol)[:, None]
    spread = np.where(near, np.abs(vals - ref[:, None]), 0.0).max(axis=1)
    same_value = spread <= EPS32 * np.abs(ref)
    strict = decidable | allzero | same_value
    print(f"{what}: atol {atol:.3e}, decidable max err {err[strict].max():.3e} ({err[strict].max() / atol:.3f} atol), "
          f"undecidable {np.mean(~strict):.4%}")
    assert err[strict].max() <= atol, f"{what}: decidable samples, max err {err[strict].max():.3e} > atol {atol:.3e}"
    rest = np.flatnonzero(~strict)
    if rest.size:
        d = np.abs(out[rest].astype(np.complex128)[:, None] - vals[rest])
        best = np.where(near[rest], d, np.inf).min(axis=1)
        print(f"{what}: undecidable max err to a near-maximum bin {best.max():.3e}")
        assert best.max() <= atol, f"{what}: undecidable samples, {best.max():.3e} > atol {atol:.3e}"
    return float(np.mean(~strict))


# ------------------------------------------------------------------ NoiseBlanker
def bursty(rng, n):
    """Level steps over 60 dB, a run of exact zeros and single-sample spikes x50 (as test_loops.py)."""
    env = np.repeat(10.0 ** rng.uniform(-3, 0, n // 500 + 1), 500)[:n]
    x = (iq(rng, n) * env.astype(np.float32)).astype(np.complex64)
    x[n // 3:n // 3 + 700] = 0
    x[rng.integers(0, n, 12)] *= 50
    return x


class NoiseBlankerRef:
    """noise_blanker.h:38-57 over np.float32 scalars, operation for operation."""

    def __init__(self, rate, level):
        self.amp = np.float32(1.0)
        self.set(rate, level)

    def set(self, rate, level):
        self.rate = np.float32(rate)
        self.inv = np.float32(1.0) - self.rate
        self.level = np.float32(level)

    def reset(self):
        self.amp = np.float32(1.0)

    def process(self, x):
        re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
        a = np.sqrt((re * re) + (im * im))                  # complex_t::amplitude(), f32 throughout
        g = np.ones(len(x), np.float32)
        amp, rate, inv, level, one = self.amp, self.rate, self.inv, self.level, np.float32(1.0)
        for i in range(len(x)):
            ia = a[i]
            if ia != 0:
                amp = (amp * inv) + (ia * rate)
                excess = ia / amp
                if excess > level:
                    g[i] = one / excess
        self.amp = amp
        out = np.empty(len(x), np.complex64)
        out.real, out.imag = re * g, im * g
        return out


# ------------------------------------------------------------------ Squelch
SQ_N = 1000


class SquelchRef:
    """squelch.h:33-63 with the level kept in fp64; cnt per object (the port's deliberate deviation:
    squelch.h:40 declares it static, one counter for every Squelch of the process)."""

    def __init__(self, level):
        self.L = float(np.float32(level))
        self.muted, self.cnt = False, 0
        self.levels = []

    def set_level(self, level):
        self.L = float(np.float32(level))

    def process(self, x):
        level = 20.0 * np.log10(np.abs(x.astype(np.complex128)).sum() / len(x))
        self.levels.append((level, self.L))
        if self.muted:
            if level < self.L or self.cnt <= 0:
                self.cnt = 10
            else:
                self.cnt -= 1
                if self.cnt == 0:
                    self.muted = False
        elif level < self.L - 1.0:
            self.cnt = 0
            self.muted = True
        return np.zeros_like(x) if self.muted else x.copy()


def noise_at(rng, db):
    x = (rng.standard_normal(SQ_N) + 1j * rng.standard_normal(SQ_N)) / np.sqrt(2.0)
    x *= 10.0 ** (db / 20.0) / np.abs(x).mean()
    return x.astype(np.complex64)


SQ_SEQUENCE = [-20.0, -45.0] + [-20.0] * 10 + [-20.0, -30.5, -45.0] + [-20.0] * 3 + [-40.0] + [-20.0] * 11


def squelch_blocks(seed=99):
    rng = np.random.default_rng(seed)
    return [noise_at(rng, db) for db in SQ_SEQUENCE]
