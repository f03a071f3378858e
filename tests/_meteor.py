"""Numpy float32 restatements of the reference's carrier loops and its Meteor (LRPT) demodulator, and the
seeded signals their tests use (a plain helper module: importable without a GPU).

One scalar operation per reference operation, in the reference's order, file:line cited (loop/ = core/src/dsp/loop,
meteor_ = decoder_modules/meteor_demodulator/src). Built on _restated.py's critically_damped, ref_fir32, ref_fast_agc
and RefMM. The per-sample loops carry a leading batch axis (one independent stream per row). Every loop takes
`trig`: cs(p) -> (cosf, sinf) and atan2(y, x) -> atan2f, in numpy's float32 (trig32) or in fp64 rounded once
(trig64); the gap between the two runs is the loop's own sensitivity to the last bit of its libm.
tests/test_meteor_ref.py holds these functions to the reference's own code (tests/golden/ref_meteor_*.npz, made
by tools/gen_ref_fixtures.py meteor_fixtures); the device tests hold the kernels to these functions."""
import functools
from types import SimpleNamespace

import numpy as np

from sdrpp_amd import dsp
from _restated import (f32, N, FL_M_PI, step, critically_damped, ref_fast_agc, ref_fir32, RefMM, trig32 as _cs32,
                       trig64 as _cs64, rrc64, parts)

trig32 = SimpleNamespace(name="trig32", cs=_cs32, atan2=lambda y, x: np.arctan2(y, x))
trig64 = SimpleNamespace(name="trig64", cs=_cs64,
                         atan2=lambda y, x: np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(f32))

TWO_PI = f32(2.0) * FL_M_PI                                      # 2.0f * FL_M_PI (math/normalize_phase.h:7-8)
# meteor_costas.h:36-39: const float = a double literal
PHASES = np.array([0.47439988279190737, 2.1777839908413044, 3.8682349942715186, -0.29067248091319986]).astype(f32)
SEEDS = range(8)


def normalize_phase(d):                                         # math/normalize_phase.h:6-10
    return np.where(d > FL_M_PI, d - TWO_PI, np.where(d <= -FL_M_PI, d + TWO_PI, d)).astype(f32)


class Pcl:
    """PhaseControlLoop<float> as loop/pll.h:15-25 sets it up (phase_control_loop.h:16-29), B streams."""

    def __init__(self, B, bandwidth, init_phase=0.0, init_freq=0.0, min_freq=-FL_M_PI, max_freq=FL_M_PI):
        self.alpha, self.beta = critically_damped(bandwidth)    # pll.h:20-21
        self.min_freq, self.max_freq = f32(min_freq), f32(max_freq)
        self.init_phase, self.init_freq, self.B = f32(init_phase), f32(init_freq), B
        self.delta = FL_M_PI - (-FL_M_PI)                       # phase_control_loop.h:28
        self.reset()

    def reset(self):                                            # pll.h:55-62
        self.phase, self.freq = np.full(self.B, self.init_phase, f32), np.full(self.B, self.init_freq, f32)

    def advance(self, err):                                     # phase_control_loop.h:58-66
        freq = self.freq + self.beta * err                      # :60
        self.freq = np.where(freq > self.max_freq, self.max_freq, np.where(freq < self.min_freq, self.min_freq, freq))   # :78-79
        phase = self.phase + (self.freq + (self.alpha * err))   # :64
        while np.any(phase > FL_M_PI):                          # :83-84
            phase = np.where(phase > FL_M_PI, phase - self.delta, phase)
        while np.any(phase < -FL_M_PI):
            phase = np.where(phase < -FL_M_PI, phase + self.delta, phase)
        self.phase = phase.astype(f32)


def derotate(xr, xi, c, s):                                     # types.h:23-25
    return (xr * c) - (xi * s), (xi * c) + (xr * s)


def pll_run(pcl, xr, xi, trig, carrier):
    """loop/pll.h:64-70 (carrier False) / loop/carrier_tracking_pll.h:14-20 (True) from pcl's state, which moves on."""
    yr, yi = np.empty_like(xr), np.empty_like(xi)
    for i in range(xr.shape[1]):
        if carrier:
            c, s = trig.cs(-pcl.phase)                          # carrier_tracking_pll.h:16
            yr[:, i], yi[:, i] = derotate(xr[:, i], xi[:, i], c, s)
        else:
            yr[:, i], yi[:, i] = trig.cs(pcl.phase)             # pll.h:66
        pcl.advance(normalize_phase(trig.atan2(xi[:, i], xr[:, i]) - pcl.phase))   # pll.h:67, types.h:57-59
    return yr, yi


def ref_pll(xr, xi, bandwidth, trig=trig32, **kw):
    return pll_run(Pcl(xr.shape[0], bandwidth, **kw), xr, xi, trig, False)


def ref_carrier_pll(xr, xi, bandwidth, trig=trig32, **kw):
    return pll_run(Pcl(xr.shape[0], bandwidth, **kw), xr, xi, trig, True)


def meteor_error(re, im, broken, trig):                         # meteor_costas.h:33-56
    if broken:
        phase = trig.atan2(im, re)                              # :41
        dp = [normalize_phase(phase - p) for p in PHASES]       # :42-45
        lowest = dp[0]
        for d in dp[1:]:                                        # :47-49
            lowest = np.where(np.abs(d) < np.abs(lowest), d, lowest)
        err = lowest * np.sqrt((re * re) + (im * im))           # :50, types.h:79
    else:
        err = (step(re) * im) - (step(im) * re)                 # :53
    return np.where(err < f32(-1), f32(-1), np.where(f32(1) < err, f32(1), err)).astype(f32)   # :55


def meteor_costas_run(pcl, xr, xi, broken, trig):
    """meteor_costas.h:24-30 from pcl's state, which moves on."""
    yr, yi = np.empty_like(xr), np.empty_like(xi)
    for i in range(xr.shape[1]):
        c, s = trig.cs(-pcl.phase)                              # :26
        re, im = derotate(xr[:, i], xi[:, i], c, s)
        yr[:, i], yi[:, i] = re, im
        pcl.advance(meteor_error(re, im, broken, trig))         # :27
    return yr, yi


def ref_meteor_costas(xr, xi, bandwidth, broken, trig=trig32, switch_at=None, **kw):
    """One run; switch_at: setBrokenModulation(not broken) before that sample (the state is kept)."""
    pcl = Pcl(xr.shape[0], bandwidth, **kw)
    if switch_at is None:
        return meteor_costas_run(pcl, xr, xi, broken, trig)
    a = meteor_costas_run(pcl, xr[:, :switch_at], xi[:, :switch_at], broken, trig)
    b = meteor_costas_run(pcl, xr[:, switch_at:], xi[:, switch_at:], not broken, trig)
    return np.concatenate([a[0], b[0]], 1), np.concatenate([a[1], b[1]], 1)


class RefMeteor:
    """demod::Meteor (meteor_demod.h:24-43, 139-167) for B streams; process() takes [B, n] and returns one symbol
    array per stream."""

    def __init__(self, B, symbolrate, samplerate, rrc_taps, rrc_beta, agc_rate, costas_bandwidth, broken, oqpsk,
                 omega_gain, mu_gain, omega_rel_limit=0.01, trig=trig32):
        self.B, self.trig, self.broken, self.oqpsk = B, trig, bool(broken), bool(oqpsk)
        self.taps = dsp.root_raised_cosine(rrc_taps, rrc_beta, samplerate / symbolrate)   # :31
        self.agc = (1.0, 10e6, agc_rate)                        # :33
        self.pcl = Pcl(B, costas_bandwidth)                     # :34
        self.mm = [RefMM(samplerate / symbolrate, omega_gain, mu_gain, omega_rel_limit, cplx=True) for _ in range(B)]   # :35
        self.last_i = np.zeros(B, f32)                          # :188
        self.reset()

    def reset(self):                                            # :139-148: the four blocks, not lastI
        self.hist = np.zeros((self.B, len(self.taps) - 1), np.complex64)   # fir.h:49-53
        self.gain = np.full(self.B, f32(1.0))                   # fast_agc.h:54-58
        self.pcl.reset()
        for m in self.mm:
            m.reset()                                           # mm.h:87-98: the history stays

    def process(self, x):
        x = np.atleast_2d(x).astype(np.complex64)
        n = x.shape[1]
        if n:
            buf = np.concatenate([self.hist, x], 1)
            T = len(self.taps)
            f = np.stack([ref_fir32(b, self.taps)[T - 1:] for b in buf])   # :151, fir.h:62-83 over [history || x]
            self.hist = buf[:, n:]
            ar, ai, self.gain = ref_fast_agc(*parts(f), *self.agc, self.gain)   # :152
            cr, ci = meteor_costas_run(self.pcl, ar, ai, self.broken, self.trig)   # :153
            if self.oqpsk:                                      # :155-161
                ci = np.concatenate([self.last_i[:, None], ci], 1)
                self.last_i, ci = ci[:, -1].copy(), ci[:, :-1]
        else:
            cr = ci = np.zeros((self.B, 0), f32)
        return [m.process((cr[k] + 1j * ci[k]).astype(np.complex64)) for k, m in enumerate(self.mm)]   # :166

    def run(self, x, ops):
        """The probe's call list over x [B, n]: counts = process() calls, "r", "b0" / "b1", "q0" / "q1".
        Returns (per-call counts [B, calls], the symbols per stream)."""
        x = np.atleast_2d(x)
        at, counts, out = 0, [], [[] for _ in range(self.B)]
        for op in ops:
            if isinstance(op, str):
                if op == "r":
                    self.reset()
                elif op[0] == "b":
                    self.broken = op[1] == "1"
                else:
                    self.oqpsk = op[1] == "1"
                continue
            y = self.process(x[:, at:at + op])
            at += op
            counts.append([len(v) for v in y])
            for k, v in enumerate(y):
                out[k].append(v)
        return np.array(counts, np.int32).T, [np.concatenate(v) for v in out]


def ref_meteor(x, args, trig=trig32, ops=None):
    """One stream through RefMeteor(*args): (per-call counts, symbols)."""
    c, y = RefMeteor(1, *args, trig=trig).run(x, [len(x)] if ops is None else ops)
    return c[0], y[0]


# ------------------------------------------------------------------ signals
# main.cpp:66: demod.init(vfo->output, 72000, 150000, 33, 0.6, 0.1, 0.005, brokenModulation, oqpsk, 1e-6, 0.01)
def meteor_args(broken, oqpsk, agc_rate=0.1, costas_bandwidth=0.005):
    return (72000.0, 150000.0, 33, 0.6, agc_rate, costas_bandwidth, bool(broken), bool(oqpsk), 1e-6, 0.01, 0.01)


UP, DOWN = 25, 12                                                # 150000 / 72000 = 25 / 12 samples per symbol
NSYM = N * DOWN // UP                                            # 5760 symbols in N samples


def lrpt_signal(seed, kind="qpsk", amp=0.05, cfo=2e-4, phase=0.3, snr_db=25.0, n=N):
    """RRC(beta 0.6)-shaped 4-point symbols at 25/12 samples per symbol: shaped at 25 samples per symbol with the
    33-tap filter's span (33 x 12 taps + 1), every 12th sample kept. kind: "qpsk" (points at pi/4 + q pi/2),
    "broken" (at meteor_costas.h's PHASE[q]) or "oqpsk" (qpsk with the Q arm one OUTPUT sample late, what
    meteor_demod.h:155-161 undoes). rms amplitude `amp`, carrier offset `cfo` cycles/sample, complex Gaussian noise
    at snr_db. Returns (x complex64 [n], q)."""
    rng = np.random.default_rng(seed)
    nsym = n * DOWN // UP + 2
    q = rng.integers(0, 4, nsym)
    sym = np.exp(1j * PHASES.astype(np.float64)[q]) if kind == "broken" else np.exp(1j * (np.pi / 4 + q * np.pi / 2))
    up = np.zeros(nsym * UP, np.complex128)
    up[::UP] = sym
    s = np.convolve(up, rrc64(33 * DOWN + 1, 0.6, UP))[:nsym * UP][::DOWN][:n]
    if kind == "oqpsk":
        s = s.real + 1j * np.concatenate([[0.0], s.imag[:-1]])
    s *= amp / np.sqrt(np.mean(np.abs(s[200:]) ** 2))
    s = s * np.exp(1j * (2 * np.pi * cfo * np.arange(n) + phase))
    sigma = np.sqrt(np.mean(np.abs(s) ** 2) / 10 ** (snr_db / 10) / 2)
    s = s + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return s.astype(np.complex64), q[:n * DOWN // UP]


def bank_streams(S, kind="qpsk", n=N, seed0=300, unit=False):
    """([n, S], the transmitted symbols per stream): streams that differ in seed, amplitude (unit: all at rms 1, what an
    AGC hands a loop), carrier offset and phase, so that swapped streams fail."""
    xs, qs = [], []
    for k in range(S):
        x, q = lrpt_signal(seed0 + k, kind, amp=1.0 if unit else 0.03 + 0.01 * (k % 5), cfo=1e-4 * ((k % 7) - 3),
                           phase=0.2 + 0.37 * k, n=n)
        xs.append(x)
        qs.append(q)
    return np.ascontiguousarray(np.stack(xs, 1)), qs


def bank_carriers(S, n=N, seed0=400):
    """[n, S]: noisy carriers that differ in seed, frequency and amplitude."""
    return np.ascontiguousarray(np.stack([carrier(seed0 + k, w=0.02 + 0.005 * (k % 9), amp=0.3 + 0.1 * (k % 6), n=n)
                                          for k in range(S)], 1))


# ------------------------------------------------- the fixture cases (tools/gen_ref_fixtures.py meteor_fixtures)
# The loops alone. PLL and CarrierTrackingPLL track a noisy carrier at 0.05 rad/sample; MeteorCostas takes the LRPT
# signals at unit rms (what the AGC hands it). 8 seeds per case: S is over all of them, seed [0] is the fixture's.
LOOP_BW = 0.01                                                  # PLL / CarrierTrackingPLL bandwidth
COSTAS_BW = 0.005                                               # main.cpp:66
LOOP_OPS = [3001, "r", 2999, 6000]                              # reset() between calls
COSTAS_OPS = [4000, "b1", 4000, "r", 4000]                      # setBrokenModulation(true), reset() between calls
# the demodulator: 0-sample calls, setOQPSK off and on (the stale lastI), reset(), setBrokenModulation
METEOR_OPS = [1, 6, 7, 0, 2986, "q0", 2000, "q1", 0, 2000, "r", 2000, "b1", 3000]
assert sum(c for c in LOOP_OPS + COSTAS_OPS + METEOR_OPS if not isinstance(c, str)) == 3 * N


def carrier(seed, w=0.05, amp=0.5, snr_db=30.0, n=N):
    """A carrier at w rad/sample, phase 0.4, complex Gaussian noise at snr_db."""
    rng = np.random.default_rng(seed)
    sigma = amp * np.sqrt(1.0 / 10 ** (snr_db / 10) / 2)
    x = amp * np.exp(1j * (w * np.arange(n) + 0.4)) + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def unit_lrpt(seed, kind):
    return (lrpt_signal(seed, kind)[0] / f32(0.05)).astype(np.complex64)


# Seeds of the demodulator cases, found by tools/gen_ref_fixtures.py --meteor-search. MM decides an interpolator phase
# per symbol, floor(u) of u = phase * 128 (mm.h:111), and with it the offset. The phase before the floor is
# ~2.08 + a fraction, so u moves in steps of 128 ulp(2.08) = 3.05e-5, and the rounding of every step walks it by a
# few such steps between two runs that differ in the last bit of the loop's libm (S_u of the two restatements:
# 1e-4 .. 4e-4). Where u lies that close to an integer, one run takes the neighbouring interpolator phase: the
# symbol differs by ~5e-3 of the radius and the loop goes another way from there. That is a property of MM on
# the stream, not of the code under test, so every case's 8 streams are streams on which the two restatements agree on
# every count and decision (S then measures the arithmetic, not a flip), and the first, the fixture's and the
# device's, is the one of seeds 0 .. 47 whose u stays farthest from an integer: at least MM_MARGIN, 5 steps of u
# (mm_margin below; the CPU tests assert all of this). The first 16 symbols, made of the zero history, do not
# count: their error term is absorbed in the phase (|y| < 1e-6), which follows k * omega alike in every run.
MM_MARGIN = 1.5e-4
MM_SETTLE = 16
METEOR_SEEDS = {"qpsk": [30, 5, 6, 7, 8, 10, 12, 13], "broken": [4, 3, 5, 8, 12, 13, 17, 19],
                "oqpsk": [17, 6, 7, 8, 9, 11, 12, 14], "ops": [13, 0, 3, 4, 6, 8, 11, 15]}
METEOR_CASES = {"qpsk": (False, False), "broken": (True, False), "oqpsk": (False, True)}   # kind -> (broken, oqpsk)
OPS_KIND, OPS_START = "oqpsk", (False, True)                    # the ops case: the OQPSK signal, oqpsk on at first


def mm_margin(xs, args, ops, trig):
    """(counts [B, calls], symbols per stream, per stream the smallest distance of MM's phase * P to an integer)."""
    r = RefMeteor(len(xs), *args, trig=trig)
    for m in r.mm:
        m.trace = []
    c, y = r.run(xs, ops)
    d = []
    for m in r.mm:
        u = np.array(m.trace, np.float64)[MM_SETTLE:]
        u = u[u != 0.0]                                         # (phase = 0 exactly: the state after reset, mm.h:87-98)
        d.append(float(np.abs(u - np.round(u)).min()))
    return c, y, np.array(d)


def meteor_case(name):
    """(the case's 8 streams [8, N], Meteor arguments, ops)."""
    kind = OPS_KIND if name == "ops" else name
    b, o = OPS_START if name == "ops" else METEOR_CASES[name]
    xs = np.stack([lrpt_signal(s, kind)[0] for s in METEOR_SEEDS[name]])
    return xs, meteor_args(b, o), (METEOR_OPS if name == "ops" else [N])


@functools.lru_cache(maxsize=None)
def meteor_ref_and_S(name):
    """Computed once per process; nothing may write to the arrays. The fp64-trig restatement of the case's first stream, S over its 8 streams (the gap of the two restatements
    over the symbols, whose counts must agree), and the MM margin of the first stream in the two runs."""
    xs, args, ops = meteor_case(name)
    ca, ya, da = mm_margin(xs, args, ops, trig32)
    cb, yb, db = mm_margin(xs, args, ops, trig64)
    assert np.array_equal(ca, cb), f"{name}: the two restatements disagree on a count"
    S = max(gap(a, b) for a, b in zip(ya, yb))
    return dict(x=xs[0], counts=cb[0], ref=yb[0], ref32=ya[0], S=S, bar=bar_of(S, yb[0]), margin=float(min(da[0], db[0])))


SWITCH_AT = 4000                                                 # setBrokenModulation(true) before this sample
# name -> (the signal of seed s, run(xr, xi, trig)): the loops alone, as the fixtures and the device tests run them
LOOP_CASES = {
    "pll": (carrier, lambda xr, xi, trig: ref_pll(xr, xi, LOOP_BW, trig)),
    "carrier_pll": (carrier, lambda xr, xi, trig: ref_carrier_pll(xr, xi, LOOP_BW, trig)),
    "meteor_costas_plain": (lambda s: unit_lrpt(s, "qpsk"), lambda xr, xi, trig: ref_meteor_costas(xr, xi, COSTAS_BW, False, trig)),
    "meteor_costas_broken": (lambda s: unit_lrpt(s, "broken"), lambda xr, xi, trig: ref_meteor_costas(xr, xi, COSTAS_BW, True, trig)),
    "meteor_costas_switch": (lambda s: unit_lrpt(s, "broken"),
                             lambda xr, xi, trig: ref_meteor_costas(xr, xi, COSTAS_BW, False, trig, switch_at=SWITCH_AT)),
}


def bar_of(S, ref):
    """The project's sensitivity bar (test_symsync.py): 16 max(S, 4 eps32 max|y|)."""
    return 16 * max(S, 4 * float(np.finfo(f32).eps) * float(np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def loop_ref_and_S(name):
    """The fp64-trig restatement of seed 0's stream, the fp32-trig one, and S over the 8 seeds. Computed once per
    process; nothing may write to the arrays."""
    signal, run = LOOP_CASES[name]
    xs = np.stack([signal(s) for s in SEEDS])
    xr, xi = parts(xs)
    a, b = run(xr, xi, trig32), run(xr, xi, trig64)
    S = float(max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()))
    ref, ref32 = (b[0][0] + 1j * b[1][0]).astype(np.complex64), (a[0][0] + 1j * a[1][0]).astype(np.complex64)
    return dict(x=xs[0], ref=ref, ref32=ref32, S=S, bar=bar_of(S, ref))


def gap(a, b):
    """The largest difference of a component of two complex arrays."""
    return float(max(np.abs(a.real - b.real).max(), np.abs(a.imag - b.imag).max()))


def nearest_phase(z):
    """The index of the PHASE constant nearest a symbol's angle (the broken-modulation decision)."""
    d = np.angle(z)[:, None] - PHASES.astype(np.float64)[None, :]
    return np.argmin(np.abs((d + np.pi) % (2 * np.pi) - np.pi), axis=1)


def sensitivity(run):
    """S of a loop: the largest gap between run(trig32) and run(trig64), each (re, im) over the 8 seeds."""
    a, b = run(trig32), run(trig64)
    return float(max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())), b
