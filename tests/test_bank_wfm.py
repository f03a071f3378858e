"""Broadcast-FM banks on the device (libsdrgpu, HIP): the complex-tap FIR, the stereo de-emphasis, the stereo decoder
inside BankBroadcastFM, over S streams in the channelizer's layout x[m, k].

Bars, none from a bank's own numbers:
* Complex FIR -- every column within 8 eps sqrt(T) sum(|h_re| + |h_im|) max|x| of the fp64 correlation of that column
  (the project's FIR bar, _util.fir_atol, with two products per component); the tiled and the direct kernel, a whole
  run and a cut one give the same bits; a unit impulse returns the taps, exactly; float32 input equals complex64 input
  with zero imaginary parts; with real taps it is BankFIR: both sum the same products in the same order, and each is
  within fir_atol of the fp64 sum, so they differ by 2 fir_atol at most.
* Stereo de-emphasis -- every column bit-identical to dsp.Deemphasis(50e-6, 48000, True) fed that column.
* BankBroadcastFM, stereo and mono, low-pass on and off -- bit-identical to its public stages run one after another;
  column k bit-identical to a bank of one stream fed column k in the same calls; whole and cut runs bit-identical; the
  first run's bits after reset; every column and channel within 2e-5 max(max|ref|, 1) of oracle.BroadcastFMStereo fed the
  same calls (the bar and the reason of tests/test_loops.py test_broadcast_fm_stereo_vs_oracle); mono: l == r.
* Known answers over rows 2200..4199 (tests/_bank_wfm.py): (l + r) / 2 at the stream's L tone is 0.45 * 75 / 100 = 0.3375
  within 5 % (the CPU oracle: 0.3263 to 0.3468 over the 130 streams); (l - r) / 2 at the L tone >= 0.08 (oracle 0.110
  to 0.116; mono: exactly 0); its ratio to that at the R tone is 1 / 0.6 within 10 % (oracle 1.594 to 1.743).
* Channelizer -> BankBroadcastFM -> BankRationalResampler -> stereo BankDeemphasis by device pointer equals the same banks
  fed a host copy.
* Shapes: S in {1, 63, 64, 65, 130}, 4200 rows, fs 240 kS/s, deviation 100 kHz. CUTS: one row; 152 / 153 / 154, a call's end
  before, on and after the 153-row delay line (305 pilot taps); an empty call; 31 / 32 / 33 across a BANK_F tile;
  1024 / 1025 across a tiled-FIR tile; the rest.
The parity summary goes to bank_wfm_parity.jsonl through write_report.
"""
import contextlib
import math
import os

import numpy as np
import pytest

import oracle
import sdrpp_amd
from sdrpp_amd import dsp
from _util import EPS32, fir_atol, iq, write_report
from _restated import same
from _bank_wfm import FS, DEVIATION, FRAMES, stereo_bank, tone_amplitude, l_tone, r_tone
from test_banks import SHAPES, SMAX, cached, noise_bank
from test_bank_rate import call, run_cuts, streams_differ

pytestmark = pytest.mark.gpu

f32 = np.float32
c64 = np.complex64
CUTS = [1, 152, 153, 154, 0, 31, 32, 33, 1024, 1025]
CUTS = CUTS + [FRAMES - sum(CUTS)]
assert FRAMES == 4200 and CUTS[-1] > 0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"


@contextlib.contextmanager
def form(tiled):
    """complex-tap FIR banks created inside run the tiled or the direct kernel: the knob is read at creation"""
    keys = ("SDRGPU_TUNING", "SDRGPU_BANK_CFIR_TILED")
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update(SDRGPU_TUNING="1", SDRGPU_BANK_CFIR_TILED="1" if tiled else "0")
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def whole_and_cut(make, X, what):
    y = call(make(), X)
    z, _ = run_cuts(make(), X, CUTS)
    assert same(y, z), f"{what}: in calls differs from one call"
    return y


# ------------------------------------------------------------- 1. complex-tap FIR
def pilot_taps():
    return dsp.band_pass(18750, 19250, 3000, FS, odd=True, complex_taps=True)


CFIR_TAPS = {"one": lambda: np.array([0.75 - 0.5j], c64),
             "ramp8": lambda: ((np.arange(1, 9) / 8.0) * np.exp(1j * 0.9 * np.arange(8))).astype(c64),
             "pilot305": pilot_taps}
CFIR_T = {"one": 1, "ramp8": 8, "pilot305": 305}


def cfir_atol(taps, x):
    """8 eps sqrt(T) sum(|h_re| + |h_im|) max|x|: fir_atol with the two products of a component"""
    return fir_atol(np.abs(taps.real) + np.abs(taps.imag), x)


def fir64(x, taps):
    """the fp64 correlation over [T - 1 zeros || x], taps not reversed (filter/fir.h:62-83)"""
    return np.convolve(np.asarray(x, np.complex128), np.asarray(taps, np.complex128)[::-1])[:len(x)]


@pytest.mark.parametrize("real_input", [False, True])
@pytest.mark.parametrize("name", sorted(CFIR_TAPS))
@pytest.mark.parametrize("S", SHAPES)
def test_complex_fir(S, name, real_input):
    taps = CFIR_TAPS[name]()
    assert len(taps) == CFIR_T[name] and taps.dtype == c64
    X = noise_bank(not real_input)[:, :S]
    what = f"complex fir {name} S={S} real_input={real_input}"
    outs = []
    for tiled in (True, False):
        with form(tiled):
            outs.append(whole_and_cut(lambda: dsp.BankFIRComplex(S, taps, real_input=real_input), X, f"{what} tiled={tiled}"))
    Y = outs[0]
    assert Y.shape == (FRAMES, S) and Y.dtype == c64
    assert same(outs[0], outs[1]), f"{what}: the tiled and the direct kernel differ"
    streams_differ(Y)
    worst = 0.0
    for k in range(S):
        err, bound = np.abs(Y[:, k] - fir64(X[:, k], taps)).max(), cfir_atol(taps, X[:, k])
        worst = max(worst, err / bound)
        assert err <= bound, f"{what}: stream {k} max abs err {err:.3e} > {bound:.3e}"
    if real_input:
        Z = call(dsp.BankFIRComplex(S, taps), X.astype(c64))
        assert np.array_equal(Y, Z), f"{what}: differs from complex input with zero imaginary parts"
    write_report("bank_wfm_parity", {"test": "complex_fir", "taps": name, "S": S, "frames": FRAMES, "real_input": real_input,
                                     "max_err_over_bound": worst})


@pytest.mark.parametrize("real_input", [False, True])
@pytest.mark.parametrize("name", sorted(CFIR_TAPS))
def test_complex_fir_impulse_returns_the_taps(name, real_input):
    taps = CFIR_TAPS[name]()
    T, S = len(taps), SMAX
    X = np.zeros((FRAMES, S), f32 if real_input else c64)
    want = np.zeros((FRAMES, S), c64)
    for k in range(S):
        X[k % 11, k] = 1
        want[k % 11:k % 11 + T, k] = taps[::-1]                  # out[m] = taps[p + T - 1 - m]: a correlation
    for tiled in (True, False):
        with form(tiled):
            Y = whole_and_cut(lambda: dsp.BankFIRComplex(S, taps, real_input=real_input), X, f"impulse {name} tiled={tiled}")
        assert np.array_equal(Y, want), f"impulse {name} real_input={real_input} tiled={tiled}: not the taps"


@pytest.mark.parametrize("S", [65, 130])
def test_complex_fir_with_real_taps_is_bank_fir(S):
    taps = dsp.low_pass(15000, 4000, FS)
    X = noise_bank(True)[:, :S]
    a = call(dsp.BankFIRComplex(S, taps.astype(c64)), X)
    b = call(dsp.BankFIR(S, taps), X)
    worst = 0.0
    for k in range(S):
        err, bound = np.abs(a[:, k] - b[:, k]).max(), 2 * fir_atol(taps, X[:, k])
        worst = max(worst, err / bound)
        assert err <= bound, f"stream {k}: max abs difference {err:.3e} > {bound:.3e}"
    write_report("bank_wfm_parity", {"test": "complex_fir_real_taps_vs_bank_fir", "S": S, "max_diff_over_bound": worst})


# --------------------------------------------------------- 2. stereo de-emphasis
@pytest.mark.parametrize("S", SHAPES)
def test_stereo_deemphasis_is_the_single_stream_block(S):
    X = noise_bank(True)
    refs = cached(("deemp2",), lambda: [dsp.Deemphasis(50e-6, 48000, True).process(np.ascontiguousarray(X[:, k]).view(dsp.STEREO))
                                         .view(c64).copy() for k in range(SMAX)])
    Y = whole_and_cut(lambda: dsp.BankDeemphasis(S, 50e-6, 48000, stereo=True), X[:, :S], f"stereo de-emphasis S={S}")
    assert Y.dtype == c64
    streams_differ(Y)
    for k in range(S):
        assert same(np.ascontiguousarray(Y[:, k]), refs[k]), f"stream {k} differs from dsp.Deemphasis(stereo) fed that column"
    write_report("bank_wfm_parity", {"test": "stereo_deemphasis", "S": S, "frames": FRAMES, "bit_identical": True})


def test_mono_deemphasis_keeps_its_signature_and_bits():
    X = noise_bank(False)[:, :65]
    Y = call(dsp.BankDeemphasis(65, 50e-6, 48000), X)
    assert Y.dtype == f32
    for k in (0, 63, 64):
        assert same(np.ascontiguousarray(Y[:, k]), dsp.Deemphasis(50e-6, 48000).process(np.ascontiguousarray(X[:, k])))


# -------------------------------------------------------------- 3. BankBroadcastFM
MODES = [(True, True), (True, False), (False, True), (False, False)]   # (stereo, low_pass)


def fm_input():
    return cached(("wfm_in",), lambda: stereo_bank(SMAX))


def make_fm(S, stereo, low_pass):
    return dsp.BankBroadcastFM(S, DEVIATION, FS, low_pass=low_pass, stereo=stereo)


def run_stages(S, stereo, low_pass, X):
    """the public stages one after another, each over the same CUTS"""
    taps = dsp.low_pass(15000, 4000, FS)
    Y, _ = run_cuts(dsp.BankQuadrature(S, 2.0 * math.pi * (DEVIATION / FS)), X, CUTS)
    if stereo:
        Y, _ = run_cuts(dsp.BankStereoDecoder(S, FS), Y, CUTS)
        if low_pass:
            Y, _ = run_cuts(dsp.BankFIR(S, taps), Y, CUTS)
        return Y
    if low_pass:
        Y, _ = run_cuts(dsp.BankFIR(S, taps, complex_data=False), Y, CUTS)
    return np.ascontiguousarray(np.stack([Y, Y], axis=-1)).view(c64)[..., 0]   # MonoToStereo: l = r, bit for bit


def single_banks(stereo, low_pass):
    """column k through a bank of one stream, in the same calls"""
    X = fm_input()
    return cached(("wfm_one", stereo, low_pass),
                  lambda: [run_cuts(make_fm(1, stereo, low_pass), X[:, k:k + 1], CUTS)[0][:, 0].copy() for k in range(SMAX)])


def oracle_columns(stereo, low_pass):
    """column k through oracle.BroadcastFMStereo, in the same calls; (n, 2) float32 (l, r)"""
    X = fm_input()

    def one(k):
        o, i, parts = oracle.BroadcastFMStereo(DEVIATION, FS, stereo, low_pass), 0, []
        for n in CUTS:
            if n:
                y = o.process(np.ascontiguousarray(X[i:i + n, k]))
                parts.append(np.stack([y["l"], y["r"]], axis=1))
            i += n
        return np.concatenate(parts)
    return cached(("wfm_oracle", stereo, low_pass), lambda: [one(k) for k in range(SMAX)])


@pytest.mark.parametrize("stereo,low_pass", MODES)
@pytest.mark.parametrize("S", SHAPES)
def test_broadcast_fm_bank(S, stereo, low_pass):
    X = fm_input()[:, :S]
    what = f"broadcast fm S={S} stereo={stereo} low_pass={low_pass}"
    Y = whole_and_cut(lambda: make_fm(S, stereo, low_pass), X, what)
    assert Y.shape == (FRAMES, S) and Y.dtype == c64
    streams_differ(Y)
    assert same(Y, run_stages(S, stereo, low_pass, X)), f"{what}: differs from its stages run one after another"
    ones, refs = single_banks(stereo, low_pass), oracle_columns(stereo, low_pass)
    worst = 0.0
    for k in range(S):
        col = np.ascontiguousarray(Y[:, k])
        assert same(col, ones[k]), f"{what}: stream {k} differs from a bank of one stream fed that column"
        lr = col.view(f32).reshape(-1, 2)
        for ch in (0, 1):
            err = np.abs(lr[:, ch].astype(np.float64) - refs[k][:, ch]).max()
            bound = 2e-5 * max(np.abs(refs[k][:, ch]).max(), 1.0)
            worst = max(worst, err / bound)
            assert err <= bound, f"{what}: stream {k} channel {'lr'[ch]} max abs err {err:.3e} > {bound:.3e}"
    if not stereo:
        assert np.array_equal(Y.real, Y.imag), f"{what}: mono, but l != r"
    print(f"{what}: worst err / bound against the oracle {worst:.3f}")
    write_report("bank_wfm_parity", {"test": "broadcast_fm_vs_oracle", "S": S, "stereo": stereo, "low_pass": low_pass, "frames": FRAMES,
                                     "max_err_over_bound": worst, "bound": "2e-5 max(max|ref|, 1)"})


@pytest.mark.parametrize("stereo,low_pass", MODES)
def test_broadcast_fm_reset_reproduces_the_first_run(stereo, low_pass):
    S = 65
    X = fm_input()[:1001, :S]
    b = make_fm(S, stereo, low_pass)
    first = call(b, X)
    again = call(b, X)
    assert not same(again, first), "the state does not matter here: the check would show nothing"
    b.reset()
    assert same(call(b, X), first)


def test_empty_call_changes_nothing():
    S = 65
    X = fm_input()[:600, :S]
    a, b = make_fm(S, True, True), make_fm(S, True, True)
    ya = np.concatenate([call(a, X[:300]), call(a, X[300:])])
    yb = np.concatenate([call(b, X[:300]), call(b, X[:0]), call(b, X[300:])])
    assert same(ya, yb)


# ------------------------------------------------------------------ 4. known answers
def test_known_answers_stereo_and_mono():
    S = SMAX
    X = fm_input()
    Y = call(make_fm(S, True, True), X)
    M = call(make_fm(S, False, True), X)
    lo, hi, sep, ratio = [], [], [], []
    for k in range(S):
        l, r = Y[:, k].real.astype(np.float64), Y[:, k].imag.astype(np.float64)
        mid = tone_amplitude((l + r) / 2, l_tone(k))
        side_l, side_r = tone_amplitude((l - r) / 2, l_tone(k)), tone_amplitude((l - r) / 2, r_tone(k))
        lo.append(mid)
        sep.append(side_l)
        ratio.append(side_l / side_r)
        assert abs(mid - 0.3375) <= 0.05 * 0.3375, f"stream {k}: (l + r) / 2 at {l_tone(k)} Hz is {mid:.4f}, sent 0.3375"
        assert side_l >= 0.08, f"stream {k}: (l - r) / 2 at {l_tone(k)} Hz is {side_l:.4f}: no stereo difference"
        assert abs(ratio[-1] - 1 / 0.6) <= 0.1 / 0.6, f"stream {k}: L : R in (l - r) / 2 is {ratio[-1]:.3f}, sent {1 / 0.6:.3f}"
        ml, mr = M[:, k].real.astype(np.float64), M[:, k].imag.astype(np.float64)
        assert tone_amplitude((ml - mr) / 2, l_tone(k)) == 0.0, f"stream {k}: the mono path has a stereo difference"
        hi.append(tone_amplitude((ml + mr) / 2, l_tone(k)))
    write_report("bank_wfm_parity", {"test": "known_answers", "S": S, "mid_at_L": [min(lo), max(lo)], "mono_at_L": [min(hi), max(hi)],
                                     "side_at_L": [min(sep), max(sep)], "side_L_over_R": [min(ratio), max(ratio)]})


# ---------------------------------- 5. channelizer -> WFM -> 48 kS/s -> de-emphasis on the device
def test_channelizer_feeds_the_wfm_chain_by_device_pointer():
    import torch
    M, NF = 256, 1200                                           # the channelizer of test_bank_rate's pointer test
    h = dsp.windowed_sinc(16 * M, np.pi / M)
    x = iq(np.random.default_rng(5), NF * M)

    def banks():
        return dsp.BankBroadcastFM(M, DEVIATION, FS), dsp.BankRationalResampler(M, FS, 48000), \
            dsp.BankDeemphasis(M, 50e-6, 48000, stereo=True)
    fm, rr, de = banks()
    rows = rr.out_rows(NF)
    assert rows == NF // 5
    s = torch.cuda.Stream()
    d_x = torch.from_numpy(x.view(f32)).cuda()
    d_ch = torch.empty(2 * NF * M, dtype=torch.float32, device="cuda")
    d_fm = torch.empty(2 * NF * M, dtype=torch.float32, device="cuda")
    d_rr = torch.empty(2 * rows * M, dtype=torch.float32, device="cuda")
    d_y = torch.zeros(2 * rows * M, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ch = dsp.PolyphaseChannelizer(M, h)
    assert ch.process_dev(d_x.data_ptr(), NF * M, d_ch.data_ptr(), s.cuda_stream) == NF * M
    assert fm.process_dev(d_ch.data_ptr(), NF, d_fm.data_ptr(), s.cuda_stream) == NF
    assert rr.process_dev(d_fm.data_ptr(), NF, d_rr.data_ptr(), s.cuda_stream) == rows
    assert de.process_dev(d_rr.data_ptr(), rows, d_y.data_ptr(), s.cuda_stream) == rows
    s.synchronize()
    C = d_ch.cpu().numpy().view(c64).reshape(NF, M)
    Y = d_y.cpu().numpy().view(c64).reshape(rows, M)
    assert np.abs(C).max() > 0 and np.all(np.isfinite(Y.view(f32)))
    fm2, rr2, de2 = banks()
    assert same(Y, call(de2, call(rr2, call(fm2, C)))), "fed by device pointer and fed a host copy differ"
    write_report("bank_wfm_parity", {"test": "channelizer_to_wfm_chain", "channels": M, "frames": NF, "rows": rows, "bit_identical": True})


def test_pilot_filter_has_the_taps_the_cuts_assume():
    t = pilot_taps()
    assert len(t) == 305 and (len(t) - 1) // 2 + 1 == 153
    write_report("bank_wfm_parity", {"test": "bars", "cfir": "8 eps sqrt(T) sum(|h_re| + |h_im|) max|x|", "eps": float(EPS32),
                                     "oracle": "2e-5 max(max|ref|, 1)", "cuts": CUTS})
