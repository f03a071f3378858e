"""Symbol recovery on the device (libsdrgpu, HIP): FastAGC, Costas, MM, BinarySlicer,
DifferentialDecoder, and PSK / GFSK / the RDS chain composed of them, against numpy float32
restatements of the reference (one scalar operation per reference operation, file:line cited; FFTW and
VOLK are absent, so the reference's own headers cannot be compiled).

Bars:
* FastAGC, BinarySlicer, DifferentialDecoder, MM (count and every output) -- bit-exact. MM's
  interpolator dot product is VOLK's generic kernel: ascending taps, fp32, unfused.
* Costas -- the phasor is libm's cosf / sinf, which no two libms round alike. The restatement runs
  twice: with numpy's float32 cos / sin and with fp64 cos / sin rounded once to fp32. S = the largest
  gap between the two over 8 seeds of the configuration: the loop's own sensitivity to a last-bit
  change of the phasor. The device must be within 16 max(S, 4 eps32 max|y|) of the fp64-trig run (16:
  the device's libm is a third rounding of the same class and a loop amplifies differently per
  input). The bar never comes from the device's numbers. Recorded: profiles/r11/symsync_parity.json.
* PSK / GFSK / RDSBits -- bit-identical to the same blocks run one after another on the device.
* Known answers -- the restatement alone must recover the transmitted bits, then the device must.
* Every streaming test cuts its 12,000 samples into calls of [1, 6, 7, 8, 0, 1023, 1024, 1025, 4097,
  rest] (one sample, the T - 1 = 7 history edge, an empty call, the 1024-sample chunk edge) and
  requires the result bit-identical to a single call on a fresh handle.
"""
import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import dsp
from _util import EPS32

pytestmark = pytest.mark.gpu

f32 = np.float32
N = 12000
CUTS = [1, 6, 7, 8, 0, 1023, 1024, 1025, 4097]
CUTS = CUTS + [N - sum(CUTS)]
FL_M_PI = f32(3.1415926535)                                     # math/constants.h:4


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def in_calls(block, x):
    out, i = [], 0
    for c in CUTS:
        out.append(block.process(x[i:i + c]))
        i += c
    assert i == len(x) == N
    return np.concatenate(out)


def whole_and_cut(make, x, what):
    """One call on a fresh handle, and the same stream in CUTS on another: bit-identical. Returns it."""
    y = make().process(x)
    z = in_calls(make(), x)
    assert same(y, z), f"{what}: the stream in calls differs from one call"
    return y


# ------------------------------------------------------------- restatements
# The per-sample loops carry a leading batch axis (one independent stream per row): the operations are
# the reference's, in its order, on float32 arrays.
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
        self.bank = dsp.mm_interp_bank(P, T)                    # (tests/test_symsync_host.py holds it to mm.h:173-178)
        self.alpha, self.beta, self.rel = f32(mu_gain), f32(omega_gain), rel       # :32 pcl.init(_muGain, _omegaGain, ...)
        self.hr, self.hi = np.zeros(T - 1, f32), np.zeros(T - 1, f32)
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
            ph = int(np.floor(self.phase * f32(self.P)))        # :111
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


# ------------------------------------------------------------------ FastAGC
@pytest.mark.parametrize("cplx", [False, True])
def test_fast_agc_bit_exact(cplx):
    x = shaped_psk(11, 4, amp=0.05)[0]
    x[5000:5100] = 0                                            # the gain runs into maxGain
    if not cplx:
        x = np.ascontiguousarray(x.real)
    args = (1.0, 50.0, 0.1, 2.0)                                # setPoint, maxGain, rate, initGain
    make = lambda: dsp.FastAGC(*args, complex_data=cplx)
    y = whole_and_cut(make, x, "fast_agc")
    xr, xi = parts(x)
    rr, ri, g_end = ref_fast_agc(xr, xi if cplx else None, 1.0, 50.0, 0.1, f32(2.0))
    ref = (rr[0] + 1j * ri[0]).astype(np.complex64) if cplx else rr[0]
    assert same(y, ref)
    assert np.any(np.abs(ref[5000:5100]) == 0) and g_end[0] != f32(2.0)
    # get_gain, set_gain (latched at the next call), reset -> initGain
    a = make()
    a.process(x[:3000])
    g3000 = ref_fast_agc(xr[:, :3000], xi[:, :3000] if cplx else None, 1.0, 50.0, 0.1, f32(2.0))[2][0]
    assert f32(a.get_gain()) == g3000
    a.set_gain(0.25)
    assert a.get_gain() == 0.25
    rr2, ri2, g2 = ref_fast_agc(xr[:, 3000:4000], xi[:, 3000:4000] if cplx else None, 1.0, 50.0, 0.1, f32(0.25))
    ref2 = (rr2[0] + 1j * ri2[0]).astype(np.complex64) if cplx else rr2[0]
    assert same(a.process(x[3000:4000]), ref2) and f32(a.get_gain()) == g2[0]
    a.reset()
    assert a.get_gain() == 2.0
    assert same(a.process(x[:1500]), ref[:1500])


# ---------------------------------------------- slicer, differential decoder
def test_binary_slicer_bit_exact():
    x = noise(5, False)
    x[::7] = 0.0
    x[3] = -0.0
    y = whole_and_cut(dsp.BinarySlicer, x, "slicer")
    assert y.dtype == np.uint8 and same(y, ref_slicer(x))


@pytest.mark.parametrize("modulus,init", [(2, 0), (4, 3)])
def test_differential_decoder_bit_exact(modulus, init):
    x = np.random.default_rng(modulus).integers(0, modulus, N).astype(np.uint8)
    make = lambda: dsp.DifferentialDecoder(modulus, init)
    y = whole_and_cut(make, x, "differential decoder")       # (the cuts carry the last symbol across calls)
    assert same(y, ref_diff(x, modulus, init))
    d = make()
    d.process(x[:100])
    d.reset()                                                   # last <- initSym
    assert same(d.process(x[100:300]), ref_diff(x[100:300], modulus, init))


# ----------------------------------------------------------------------- MM
def mm_input(kind, cplx):
    if kind == "noise":
        return noise(77, cplx)
    x = shaped_psk(21, 4 if cplx else 2, cfo=0.0, phase=0.0 if not cplx else 0.3)[0]
    return x if cplx else np.ascontiguousarray(x.real)


MM_CASES = [(om, og, mg, 128, 8, kind)
            for om in (4.0, 5000.0 / 1187.5) for og, mg in ((2.5e-5, 0.01), (1e-6, 0.01)) for kind in ("psk", "noise")]
MM_CASES.append((4.0, 2.5e-5, 0.01, 4, 3, "psk"))


@pytest.mark.parametrize("cplx", [False, True])
def test_mm_count_and_outputs_bit_exact(cplx):
    for om, og, mg, P, T, kind in MM_CASES:
        what = f"mm cplx={cplx} omega={om} gains=({og}, {mg}) bank=({P}, {T}) {kind}"
        x = mm_input(kind, cplx)
        make = lambda: dsp.MM(om, og, mg, 0.01, P, T, complex_data=cplx)
        if T == 8:
            y = whole_and_cut(make, x, what)                    # (the cuts' history edge is T - 1 = 7)
        else:
            y = make().process(x)
        ref = RefMM(om, og, mg, 0.01, P, T, cplx).process(x)
        assert len(ref) > N / om * 0.98 - 2, what
        assert len(y) == len(ref), f"{what}: {len(y)} outputs, restatement {len(ref)}"
        assert same(y, ref), what


@pytest.mark.parametrize("cplx", [False, True])
def test_mm_reset_keeps_history_and_set_omega(cplx):
    x = mm_input("psk", cplx)
    args = (4.0, 2.5e-5, 0.01, 0.01)
    m, r = dsp.MM(*args, complex_data=cplx), RefMM(*args, cplx=cplx)
    assert m.out_count(777) == 777                              # the capacity, not the count
    assert same(m.process(x[:3001]), r.process(x[:3001]))
    m.reset()
    r.reset()                                                   # mm.h:87-98: the 7 history samples stay
    assert np.any(r.hr != 0)
    y, z = m.process(x[3001:6000]), r.process(x[3001:6000])
    assert same(y, z)
    fresh = RefMM(*args, cplx=cplx).process(x[3001:6000])
    assert not same(z[:2], fresh[:2]), "the history does not matter here: the check would show nothing"
    om2 = 5000.0 / 1187.5
    m.set_omega(om2)                                            # mm.h:40-50: offset, phase zeroed, freq and limits follow
    r.set_omega(om2)
    y, z = m.process(x[6000:]), r.process(x[6000:])
    assert same(y, z) and abs(len(z) - 6000 / om2) < 40
    with pytest.raises(sdrpp_amd.SdrGpuError):
        m.set_omega(1.0)                                        # an output would consume no input
    with pytest.raises(sdrpp_amd.SdrGpuError):
        m.set_gains(2.5e-5, 3.5)


# ------------------------------------------------------------------- Costas
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


@pytest.fixture(scope="module")
def costas_refs():
    """Per case: the fp64-trig restatement of seed 0's stream and S over the 8 seeds."""
    out = {}
    for case, c in COSTAS_CASES.items():
        xs = np.stack([costas_input(case, s) for s in SEEDS])
        xr, xi = parts(xs)
        a = ref_costas(xr, xi, c["order"], c["bandwidth"], trig=trig32, **c["kw"])
        b = ref_costas(xr, xi, c["order"], c["bandwidth"], trig=trig64, **c["kw"])
        S = float(max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()))
        out[case] = dict(x=xs[0], ref=(b[0][0] + 1j * b[1][0]).astype(np.complex64), S=S)
    return out


@pytest.mark.parametrize("case", sorted(COSTAS_CASES))
def test_costas_within_the_loops_own_sensitivity(case, costas_refs):
    c, r = COSTAS_CASES[case], costas_refs[case]
    kw = c["kw"]
    make = lambda: dsp.Costas(c["order"], c["bandwidth"], kw.get("init_phase", 0.0), kw.get("init_freq", 0.0),
                              kw.get("min_freq", -float(FL_M_PI)), kw.get("max_freq", float(FL_M_PI)))
    y = whole_and_cut(make, r["x"], case)
    ref = r["ref"]
    # the restatement locks: the loop output is the constellation, not a spinning copy of the input
    tail = ref[6000:]
    if case == "order2" or case == "rds_second_loop":
        assert np.mean(np.abs(tail.imag)) < 0.35 * np.mean(np.abs(tail.real)), "restatement did not lock"
    dev = float(max(np.abs(y.real - ref.real).max(), np.abs(y.imag - ref.imag).max()))
    bar = 16 * max(r["S"], 4 * EPS32 * float(np.abs(ref).max()))
    print(f"costas {case}: S {r['S']:.3e}, device deviation {dev:.3e}, bar {bar:.3e}")
    assert dev <= bar
    # reset -> the initial phase and frequency
    m = make()
    m.process(r["x"][:2500])
    m.reset()
    assert same(m.process(r["x"][:2000]), y[:2000])


@pytest.mark.parametrize("order", [2, 4, 8])
def test_costas_zero_input_gives_exact_zeros(order):
    y = whole_and_cut(lambda: dsp.Costas(order, 0.005), np.zeros(N, np.complex64), "costas zeros")
    assert y.shape == (N,) and not np.any(bits(y) & np.uint64(0x7FFFFFFF7FFFFFFF))   # +-0 only


def test_costas_setters():
    x = costas_input("order2", 0)
    a, b = dsp.Costas(2, 0.005), dsp.Costas(2, 0.02, 0.0, 0.0, -0.5, 0.5)
    b.set_bandwidth(0.005)
    b.set_freq_limits(-float(FL_M_PI), float(FL_M_PI))
    assert same(a.process(x[:3000]), b.process(x[:3000]))


# ------------------------------------------------- composites are their parts
def run_parts(blocks, x):
    for b in blocks:
        x = b.process(x)
    return x


def test_psk_is_its_parts():
    x = shaped_psk(31, 4, amp=0.05)[0]
    make = lambda: dsp.PSK(4, 1.0, 4.0, 31, 0.6, 0.01, 0.005, 2.5e-5, 0.01, 0.01)
    y = whole_and_cut(make, x, "psk")
    ps = [dsp.FIR(dsp.root_raised_cosine(31, 0.6, 4.0)), dsp.FastAGC(1.0, 10e6, 0.01, complex_data=True),
          dsp.Costas(4, 0.005), dsp.MM(4.0, 2.5e-5, 0.01, 0.01, complex_data=True)]
    z = run_parts(ps, x)
    assert len(y) == len(z) and abs(len(y) - 3000) <= 2 and same(y, z)


def test_mm_setters_reach_the_chain():
    """The MM setters on a PSK handle act on the chain's last block (before the first sample here)."""
    x = shaped_psk(31, 4, amp=0.05)[0][:4000]
    p = dsp.PSK(4, 1.0, 4.0, 31, 0.6, 0.01, 0.005, 2.5e-5, 0.01, 0.01)
    p.set_gains(1e-6, 0.02)
    p.set_omega_rel_limit(0.02)
    ps = [dsp.FIR(dsp.root_raised_cosine(31, 0.6, 4.0)), dsp.FastAGC(1.0, 10e6, 0.01, complex_data=True),
          dsp.Costas(4, 0.005), dsp.MM(4.0, 1e-6, 0.02, 0.02, complex_data=True)]
    assert same(p.process(x), run_parts(ps, x))


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


def test_gfsk_is_its_parts():
    x = gfsk_signal()[0]
    y = whole_and_cut(lambda: dsp.GFSK(*GFSK_ARGS), x, "gfsk")
    ps = [dsp.Quadrature(2 * np.pi * 3000.0 / 48000.0), dsp.FIR(dsp.root_raised_cosine(31, 0.6, 4.0), complex_data=False),
          dsp.MM(4.0, 2.5e-5, 0.01, 0.01)]
    z = run_parts(ps, x)
    assert y.dtype == f32 and len(y) == len(z) and same(y, z)


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


def rds_parts():
    w = W_RDS
    return [dsp.FastAGC(1.0, 1e6, 0.1, complex_data=True), dsp.Costas(2, float(f32(0.005))),
            dsp.FIR(dsp.band_pass(0, 2375, 100, 5000, complex_taps=True)),
            dsp.Costas(2, 0.01, 0.0, w, w - (w * 0.1), w + (w * 0.1))]


def test_rds_is_its_parts():
    x = rds_signal(*RDS_CASES[0])[0]
    y = whole_and_cut(dsp.RDSBits, x, "rds")
    r = dsp.RDSBits()
    assert same(r.process(x), y)
    soft = r.symbols()
    z = np.ascontiguousarray(run_parts(rds_parts(), x).real)                      # convert::ComplexToReal
    zs = dsp.MM(5000.0 / (2375.0 / 2.0), 1e-6, 0.01, 0.01).process(z)
    zb = run_parts([dsp.BinarySlicer(), dsp.DifferentialDecoder(2)], zs)
    assert y.dtype == np.uint8 and len(y) == len(zb) == len(soft)
    assert same(soft, zs) and same(y, zb)
    # the soft symbols of a later, shorter call, and of an empty one
    r.process(x[:500])
    assert abs(len(r.symbols()) - 500 / (5000.0 / 1187.5)) <= 2
    assert len(r.process(x[:0])) == 0 and len(r.symbols()) == 0


# ------------------------------------------------------------ known answers
def errors_at_best_lag(got, want, lags, lo, hi):
    """(errors, lag) of got[lag + lo : lag + hi] against want[lo:hi], the best lag."""
    best = (10 ** 9, -1)
    for lag in lags:
        g = got[lag + lo:lag + hi]
        if len(g) == hi - lo:
            best = min(best, (int(np.count_nonzero(g != want[lo:hi])), lag))
    return best


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


@pytest.mark.parametrize("f0,snr_db,seed", RDS_CASES)
def test_rds_known_answer(f0, snr_db, seed):
    x, b = rds_signal(f0, snr_db, seed)
    ref_bits, ref_soft = ref_rds_chain(x)
    hi = min(len(b), len(ref_bits)) - 80
    e, lag = errors_at_best_lag(ref_bits, b, range(80), 600, hi)
    print(f"rds f0={f0} snr={snr_db}: restatement {e} errors at lag {lag} over {hi - 600} bits, {len(ref_soft)} symbols")
    assert e == 0, "the restatement alone does not recover the bits"
    r = dsp.RDSBits()
    y = r.process(x)
    assert abs(len(y) - len(ref_bits)) <= 1
    e, lag = errors_at_best_lag(y, b, range(80), 600, hi)
    print(f"rds f0={f0} snr={snr_db}: device {e} errors at lag {lag}")
    assert e == 0


def quadrant(z):
    return (np.floor(np.angle(z) / (np.pi / 2)).astype(int)) % 4


def test_qpsk_known_answer():
    x, q = shaped_psk(61, 4, amp=0.05)
    dq = np.diff(q) % 4
    xr, xi = parts(x)
    h = dsp.root_raised_cosine(31, 0.6, 4.0)
    f = ref_fir(x, h)                                                             # psk.h:139
    fr, fi = parts(f)
    ar, ai, _ = ref_fast_agc(fr, fi, 1.0, 10e6, 0.01, f32(1.0))                  # psk.h:33, :140
    cr, ci = ref_costas(ar, ai, 4, 0.005)                                         # :34, :141
    sym = RefMM(4.0, 2.5e-5, 0.01, 0.01, cplx=True).process((cr[0] + 1j * ci[0]).astype(np.complex64))   # :35, :142
    e, lag = errors_at_best_lag(np.diff(quadrant(sym)) % 4, dq, range(40), 1000, 2800)
    print(f"qpsk: restatement {e} errors at lag {lag}, {len(sym)} symbols")
    assert e == 0, "the restatement alone does not recover the symbols"
    y = dsp.PSK(4, 1.0, 4.0, 31, 0.6, 0.01, 0.005, 2.5e-5, 0.01, 0.01).process(x)
    e, lag = errors_at_best_lag(np.diff(quadrant(y)) % 4, dq, range(40), 1000, 2800)
    print(f"qpsk: device {e} errors at lag {lag}, {len(y)} symbols")
    assert e == 0 and abs(len(y) - len(sym)) <= 1


def test_gfsk_known_answer():
    x, b = gfsk_signal()
    d = x[1:] * np.conj(x[:-1])
    q = np.concatenate([[np.angle(x[0])], np.angle(d)]) / (2 * np.pi * 3000.0 / 48000.0)   # quadrature.h:41-56
    h = dsp.root_raised_cosine(31, 0.6, 4.0)
    f = ref_fir(q.astype(f32), h)                                                 # gfsk.h:133
    soft = RefMM(4.0, 2.5e-5, 0.01, 0.01).process(f)                              # :134
    e, lag = errors_at_best_lag(ref_slicer(soft), b.astype(np.uint8), range(40), 1000, 2800)
    print(f"gfsk: restatement {e} errors at lag {lag}, {len(soft)} symbols")
    assert e == 0, "the restatement alone does not recover the bits"
    y = dsp.GFSK(*GFSK_ARGS).process(x)
    e, lag = errors_at_best_lag(ref_slicer(y), b.astype(np.uint8), range(40), 1000, 2800)
    print(f"gfsk: device {e} errors at lag {lag}, {len(y)} symbols")
    assert e == 0 and abs(len(y) - len(soft)) <= 1


# -------------------------------------------------------------- device path
def test_rds_bits_from_the_broadcast_fm_device_pointer():
    """BroadcastFM(stereo, RDS on) on an MPX-modulated IQ block; RDSBits fed the rds_dev device pointer
    on the same stream gives the bits RDSBits gives on the host copy from read_rds."""
    import ctypes
    import torch
    from sdrpp_amd import lib, check
    fs, n = 240000.0, 96000
    t = np.arange(n) / fs
    rng = np.random.default_rng(71)
    k = np.floor(1187.5 * t).astype(int)
    d = np.cumsum(rng.integers(0, 2, k.max() + 1)) % 2
    th = 2 * np.pi * 19000 * t
    mpx = 0.4 * np.sin(2 * np.pi * 1000 * t) + 0.1 * np.cos(th) + 0.05 * (2.0 * d[k] - 1.0) * np.sin(2 * np.pi * 1187.5 * t) * np.cos(3 * th)
    x = (0.5 * np.exp(1j * 2 * np.pi * 75000 * np.cumsum(mpx) / fs)).astype(np.complex64)
    fm = dsp.BroadcastFM(100000, fs, True, stereo=True, rds=True)
    s = torch.cuda.Stream()
    d_in = torch.from_numpy(x.view(f32).copy()).cuda()
    d_audio = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    d_bits = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert fm.process_dev(d_in.data_ptr(), n, d_audio.data_ptr(), s.cuda_stream) == n
    ptr, cnt = ctypes.c_void_p(), ctypes.c_int()
    check(lib.sdrgpu_broadcast_fm_rds_dev(fm._h, ctypes.byref(ptr), ctypes.byref(cnt)))
    assert cnt.value == n * 5000 // 240000
    on_dev = dsp.RDSBits()
    m = on_dev.process_dev(ptr.value, cnt.value, d_bits.data_ptr(), s.cuda_stream)   # (returns after the stream)
    got = d_bits[:m].cpu().numpy()
    host = fm.rds_output()
    assert len(host) == cnt.value
    on_host = dsp.RDSBits()
    want = on_host.process(host)
    assert m == len(want) and abs(m - cnt.value / (5000.0 / 1187.5)) <= 2
    assert same(got, want) and same(on_dev.symbols(), on_host.symbols())
