"""SSB and CW receiver banks on the device (libsdrgpu, HIP): the bank xlator, BankSSB, BankCW and the
single-stream CW block, S streams per launch in the channelizer's layout x[m, k].

The reference of every bank column is a fresh SINGLE-STREAM handle of the existing block with the same
parameters, fed that column in the same calls (the NCO's per-call table and the AGC's clip look-ahead both
depend on where calls end, so a run whole is held to handles fed whole columns and a run over CUTS to handles
fed the same cuts). Those blocks are held to the reference by tests/test_loops.py and tests/test_gpu_parity.py;
no bar here comes from a bank's own numbers.

Bars:
* BankXlator -- every column bit-identical to dsp.FrequencyXlator, whole, cut, across set_offset and after
  reset; with real=True to its real part; the impulse rows give the phasor sequence, within 2e-6 of oracle.Xlator (test_xlator_vs_fp64_nco's bar).
* BankSSB (modes 0, 1, 2, AGC on and off) -- bit-identical to BankXlator -> .real -> BankAGC with SSB's
  constants and to per-column dsp.SSB handles; at S = 65 within test_ssb_vs_oracle's bars of oracle.SSB.
* dsp.CW -- bit-identical to dsp.FrequencyXlator -> .real -> dsp.AGC(1, attack, decay, 10e6, 1.0, 1.0); BankCW
  bit-identical to its stages and to per-column dsp.CW handles, on a keyed tone that fires the AGC's look-ahead
  many times per call; against oracle.Xlator -> .real -> oracle.AGC: AGC on SSB's bar, AGC off 2e-6 max|x|.
* Channelizer -> BankSSB by device pointer, bit-identical to per-channel dsp.SSB handles.
* A call of 0 frames changes no later output.
Shapes and cuts: tests/test_banks.py (4200 rows cross row 4096, where the whole run's coarse NCO index steps).
The parity summary goes to bank_ssb_parity.jsonl through write_report.
"""
import ctypes

import numpy as np
import pytest

import oracle
import sdrpp_amd
from sdrpp_amd import dsp, lib
from _util import EPS32, assert_close_c, write_report
from _restated import same
from test_banks import FRAMES, SHAPES, SMAX, CUTS, cached, run_whole, check_columns, streams_differ
import _bank_audio as ba

pytestmark = pytest.mark.gpu

f32 = np.float32
FS = 24000.0
BW = 2800.0
TONE = 800.0
ATT, DEC = 50.0 / FS, 5.0 / FS
SSB_AGC = (1.0, ATT, DEC, 10e6, 10.0, float("inf"))             # ssb.h:27-40
CW_AGC = (1.0, ATT, DEC, 10e6, 1.0, 1.0)                         # cw.h:20
WHOLE = [FRAMES]
KA_S = 65
ORACLE_CALLS = [480, 2520, 1200]
assert FRAMES > 4096 and sum(CUTS) == FRAMES == sum(ORACLE_CALLS)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"


def rads(f):
    return 2.0 * np.pi * (f / FS)                                # math/hz_to_rads.h


def ssb_offset(mode):
    return rads(BW / 2.0 if mode == 0 else (-BW / 2.0 if mode == 1 else 0.0))   # getTranslation (ssb.h:119-126)


def col(X, k):
    return np.ascontiguousarray(X[:, k])


# ------------------------------------------------------------------- inputs
def ssb_input():
    """Stream k: the two tones of test_ssb_vs_oracle (1100 Hz at 0.2, -700 Hz at 0.05) times 0.5 + 0.25 (k mod 8),
    noise of 0.002 from seed 500 + k, rows 2000..2100 scaled x40 (am_burst_bank's burst)."""
    def make():
        t = np.arange(FRAMES)
        X = np.empty((FRAMES, SMAX), np.complex64)
        for k in range(SMAX):
            rng = np.random.default_rng(500 + k)
            x = (0.5 + 0.25 * (k % 8)) * (0.2 * np.exp(2j * np.pi * 1100 * t / FS) + 0.05 * np.exp(-2j * np.pi * 700 * t / FS))
            x = x + 0.002 * (rng.uniform(-1, 1, FRAMES) + 1j * rng.uniform(-1, 1, FRAMES))
            x[2000:2100] *= 40
            X[:, k] = x.astype(np.complex64)
        return X
    return cached(("ssb_in",), make)


def cw_input():
    """Stream k: a tone of 300 Hz keyed on and off every 2400 rows (the keying shifted by 100 (k mod 5) rows), amplitude
    0.2 (0.75 + 0.125 (k mod 5)), noise of 0.002 from seed 600 + k, rows 10..2000 at amplitude 1.5. CW's AGC starts with the
    running amplitude at 1 (cw.h:20: initial gain 1), falling by 2e-4 per row: a tone of 0.2 never rises above it in 4200 rows,
    so it is the stretch that clips the disabled branch AND fires the enabled one's look-ahead, every few cycles, in the
    calls of 7, 8, 1023 and 1024 rows of CUTS (test_cw_signal_fires_the_lookahead_often counts)."""
    def make():
        t = np.arange(FRAMES)
        X = np.empty((FRAMES, SMAX), np.complex64)
        for k in range(SMAX):
            rng = np.random.default_rng(600 + k)
            amp = np.where(((t + 100 * (k % 5)) // 2400) % 2 == 0, 0.2 * (0.75 + 0.125 * (k % 5)), 0.0)
            amp[10:2000] = 1.5
            x = amp * np.exp(1j * (2 * np.pi * 300 * t / FS + 0.2 * k))
            x = x + 0.002 * (rng.uniform(-1, 1, FRAMES) + 1j * rng.uniform(-1, 1, FRAMES))
            X[:, k] = x.astype(np.complex64)
        return X
    return cached(("cw_in",), make)


# ------------------------------------------------------------ running in calls
def in_calls(h, x, cuts, between=None):
    """x through the handle (single-stream or bank) in calls of `cuts` rows; between(h, c) runs before call c"""
    parts, i = [], 0
    for c, n in enumerate(cuts):
        if between:
            between(h, c)
        parts.append(run_whole(h, x[i:i + n])[0] if isinstance(h, dsp.Bank) else h.process(x[i:i + n]))
        i += n
    assert i == len(x)
    if isinstance(h, dsp.Bank):
        return [np.concatenate([p[k] for p in parts]) for k in range(h.streams)]
    return np.concatenate(parts)


def column_refs(key, make_single, X, cuts, between=None):
    """The reference, once per configuration: column k through a fresh single-stream handle in the same calls."""
    return cached(("colref",) + key + (tuple(cuts),), lambda: [in_calls(make_single(), col(X, k), cuts, between) for k in range(X.shape[1])])


def stage_columns(stages, X, cuts):
    """X through the stages one after another in calls of `cuts` rows; a stage is a bank or a function of the block"""
    parts, i = [], 0
    for n in cuts:
        y = X[i:i + n]
        for st in stages:
            y = st.process(y) if isinstance(st, dsp.Bank) else st(y)
        parts.append(y.copy())
        i += n
    Y = np.concatenate(parts)
    return [col(Y, k) for k in range(Y.shape[1])]


def real_part(y):
    return np.ascontiguousarray(y.real)


# -------------------------------------------------------------- 1. BankXlator
W1, W2 = rads(1400.0), rads(-650.0)


def xl1():
    return dsp.FrequencyXlator(W1)


@pytest.mark.parametrize("S", SHAPES)
def test_bank_xlator_columns(S):
    X = ssb_input()
    for cuts in (WHOLE, CUTS):
        refs = column_refs(("xl",), xl1, X, cuts)
        streams_differ(refs[:S])
        ys = in_calls(dsp.BankXlator(S, W1), X[:, :S], cuts)
        assert ys[0].dtype == np.complex64
        check_columns(ys, refs[:S], f"xlator S={S} calls={len(cuts)}")
        # translate and take the real part in one launch: the real part of the same product
        rs = in_calls(dsp.BankXlator(S, W1, real=True), X[:, :S], cuts)
        assert rs[0].dtype == f32
        check_columns(rs, [real_part(r) for r in refs[:S]], f"xlator real S={S} calls={len(cuts)}")
    whole, cut = column_refs(("xl",), xl1, X, WHOLE), column_refs(("xl",), xl1, X, CUTS)
    assert np.abs(whole[0][4096:] - cut[0][4096:]).max() < 1e-5, "the cut run lost the phase"


@pytest.mark.parametrize("S", SHAPES)
def test_bank_xlator_set_offset_keeps_the_phase_and_reset_restarts_it(S):
    X, cuts = ssb_input(), [2000, 1100, FRAMES - 3100]

    def retune(h, c):
        if c == 1:
            h.set_offset(W2)
    refs = column_refs(("xl_retune",), xl1, X, cuts, retune)
    plain = column_refs(("xl",), xl1, X, WHOLE)
    assert same(refs[0][:2000], plain[0][:2000]) and not same(refs[0][2000:], plain[0][2000:])
    # the phase is kept: right after the retune the new offset continues from the old phase (no jump back to 0)
    x0 = col(X, 0).astype(np.complex128)
    ph = np.angle(refs[0][2000] / x0[2000])
    assert abs(np.angle(np.exp(1j * (ph - 2000 * W1)))) < 1e-3 and abs(np.angle(np.exp(1j * 2000 * W1))) > 0.1
    b = dsp.BankXlator(S, W1)
    check_columns(in_calls(b, X[:, :S], cuts, retune), refs[:S], f"xlator set_offset S={S}")
    # reset: the phase starts over (with the offset as it is now, W2)
    b.reset()
    again = column_refs(("xl_w2",), lambda: dsp.FrequencyXlator(W2), X[:1000], [1000])
    check_columns(in_calls(b, X[:1000, :S], [1000]), again[:S], f"xlator reset S={S}")
    assert not same(in_calls(b, X[:1000, :S], [1000])[0], again[0]), "the phase does not matter here: the check would show nothing"


def test_bank_xlator_impulse_rows_are_the_phasors():
    S = 130
    X = np.ones((FRAMES, S), np.complex64)
    for cuts in (WHOLE, CUTS):
        ys = in_calls(dsp.BankXlator(S, W1), X, cuts)
        ref = in_calls(oracle.Xlator(W1), col(X, 0), cuts)
        assert all(same(y, ys[0]) for y in ys), "the streams of a row do not share one phasor"
        err = assert_close_c(ys[0], ref, 2e-6, "bank xlator phasors")
        assert abs(np.abs(ys[0].astype(np.complex128)) - 1).max() < 1e-6
        write_report("bank_ssb_parity", {"test": "xlator_phasors_vs_oracle", "calls": len(cuts), "max_err": float(err), "bound": 2e-6})


# ----------------------------------------------------------------- 2. BankSSB
def ssb_stages(S, mode, agc):
    return [dsp.BankXlator(S, ssb_offset(mode)), real_part, dsp.BankAGC(S, *SSB_AGC, enabled=agc)]


@pytest.mark.parametrize("agc", [True, False])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("S", SHAPES)
def test_bank_ssb_is_its_stages_and_its_single_stream_handles(S, mode, agc):
    X = ssb_input()
    args = (mode, BW, FS, agc, ATT, DEC)
    for cuts in (WHOLE, CUTS):
        what = f"ssb S={S} mode={mode} agc={agc} calls={len(cuts)}"
        ys = in_calls(dsp.BankSSB(S, *args), X[:, :S], cuts)
        assert ys[0].dtype == f32
        check_columns(ys, stage_columns(ssb_stages(S, mode, agc), X[:, :S], cuts), what + " (stages)")
        refs = column_refs(("ssb",) + args, lambda: dsp.SSB(*args), X, cuts)
        streams_differ(refs[:S])
        check_columns(ys, refs[:S], what)
    if agc:
        whole, cut = (column_refs(("ssb",) + args, lambda: dsp.SSB(*args), X, c) for c in (WHOLE, CUTS))
        assert not all(same(a, b) for a, b in zip(whole, cut)), "the calls' ends do not matter here: the cut run would show nothing"


@pytest.mark.parametrize("agc", [True, False])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_bank_ssb_vs_oracle(mode, agc):
    X = ssb_input()[:, :KA_S]
    args = (mode, BW, FS, agc, ATT, DEC)
    b, os_ = dsp.BankSSB(KA_S, *args), [oracle.SSB(*args) for _ in range(KA_S)]
    worst, clipped_min, i = 0.0, 1.0, 0
    if agc:                                                      # the burst fires every stream's look-ahead
        ev = ba.agc_events(np.stack(stage_columns(ssb_stages(KA_S, mode, True)[:2], X, ORACLE_CALLS), axis=1), ORACLE_CALLS, *SSB_AGC)
        assert {k for k, c, r, _ in ev if c == 1 and 2000 - 480 <= r < 2100 - 480} == set(range(KA_S))
    for n in ORACLE_CALLS:
        y = b.process(X[i:i + n])
        for k in range(KA_S):
            a, ref = col(y, k), os_[k].process(col(X[i:i + n], k))
            assert a.shape == ref.shape
            scale, err = max(np.abs(ref).max(), 1e-30), np.abs(a - ref)
            if agc:                                              # test_ssb_vs_oracle's bars
                print(f"ssb mode {mode} rows {i}..{i + n} stream {k}: err {err.max():.3e} scale {scale:.3e}")
                worst = max(worst, err.max() / (1e-5 * scale + 16 * EPS32 * scale))
                assert err.max() <= 1e-5 * scale + 16 * EPS32 * scale, f"mode {mode} agc on rows {i}..{i + n}: stream {k}"
            else:
                clipped = np.abs(ref) >= 10.0 * (1 - 1e-6)
                clipped_min = min(clipped_min, clipped.mean())
                assert clipped.mean() > 0.99
                worst = max(worst, err[clipped].max() / (16 * EPS32 * 10.0))
                assert np.all(err[clipped] <= 16 * EPS32 * 10.0), f"mode {mode} agc off rows {i}..{i + n}: stream {k}"
        i += n
    write_report("bank_ssb_parity", {"test": "ssb_vs_oracle", "S": KA_S, "mode": mode, "agc": agc, "max_err_over_bound": float(worst),
                                     "clipped_min": float(clipped_min)})


@pytest.mark.parametrize("S", [1, 65, 130])
def test_bank_ssb_set_gain_and_set_offset_match_the_handles(S):
    X, cuts = ssb_input(), [2000, 1100, FRAMES - 3100]
    args = (0, BW, FS, False, ATT, DEC)                         # AGC off: the fixed-gain limiter, where the gain shows

    def regain(h, c):
        if c == 1:
            if isinstance(h, dsp.Bank):
                h.set_agc_gain(2.0)
            else:
                sdrpp_amd.check(lib.sdrgpu_demod_agc_set_gain(h._h, 0, 2.0))
    refs = column_refs(("ssb_regain",) + args, lambda: dsp.SSB(*args), X, cuts, regain)
    plain = column_refs(("ssb",) + args, lambda: dsp.SSB(*args), X, cuts)
    assert same(refs[0][:2000], plain[0][:2000]) and not same(refs[0][2000:], plain[0][2000:])
    check_columns(in_calls(dsp.BankSSB(S, *args), X[:, :S], cuts, regain), refs[:S], f"ssb set_gain S={S}")

    # set_offset on the chain's xlator: the stages with the same setter
    def retune(h, c):
        if c == 1:
            h.set_offset(W2)
    b, st = dsp.BankSSB(S, 1, BW, FS, True, ATT, DEC), ssb_stages(S, 1, True)
    parts, zs, i = [], [], 0
    for c, n in enumerate(cuts):
        retune(b, c)
        retune(st[0], c)
        parts.append(b.process(X[i:i + n, :S]))
        zs.append(st[2].process(real_part(st[0].process(X[i:i + n, :S]))))
        i += n
    assert same(np.concatenate(parts), np.concatenate(zs))
    assert not same(np.concatenate(parts)[2000:], dsp.BankSSB(S, 1, BW, FS, True, ATT, DEC).process(X[:, :S])[2000:])


# ---------------------------------------------------------- 3. CW and BankCW
def cw_single_stages(agc):
    a = dsp.AGC(*CW_AGC)
    a.set_enabled(agc)
    return dsp.FrequencyXlator(rads(TONE)), a


@pytest.mark.parametrize("agc", [True, False])
def test_cw_is_xlator_real_agc(agc):
    x, cuts = col(cw_input(), 3), [2000, 1100, FRAMES - 3100]
    for calls in (WHOLE, cuts):
        g, (xl, a) = dsp.CW(TONE, agc, ATT, DEC, FS), cw_single_stages(agc)
        y = in_calls(g, x, calls)
        z = np.concatenate([a.process(real_part(xl.process(p))) for p in np.split(x, np.cumsum(calls)[:-1])])
        assert y.dtype == f32 and same(y, z), f"cw agc={agc} calls={len(calls)}"
    assert np.abs(y).max() > 0.5 and (agc or np.abs(y).max() == 1.0), "the limiter never clips"


def test_cw_set_tone_keeps_the_phase_stereo_reset_and_agc_access():
    x, cuts = col(cw_input(), 5), [2000, 1100, FRAMES - 3100]
    g, (xl, a) = dsp.CW(TONE, True, ATT, DEC, FS), cw_single_stages(True)
    parts, zs, i = [], [], 0
    for c, n in enumerate(cuts):
        if c == 1:
            g.set_tone(650.0)
            xl.set_offset(rads(650.0))
        parts.append(g.process(x[i:i + n]))
        zs.append(a.process(real_part(xl.process(x[i:i + n]))))
        i += n
    y = np.concatenate(parts)
    assert same(y, np.concatenate(zs))
    fresh = dsp.CW(TONE, True, ATT, DEC, FS)
    first = fresh.process(x)
    assert same(y[:2000], first[:2000]) and not same(y[2000:], first[2000:])
    # stereo: l == r == mono
    st = dsp.CW(TONE, True, ATT, DEC, FS, stereo=True).process(x)
    assert st.dtype == dsp.STEREO and same(np.ascontiguousarray(st["l"]), first) and same(np.ascontiguousarray(st["r"]), first)
    # reset: the phase and the AGC start over
    assert not same(fresh.process(x), first)
    fresh.reset()
    assert same(fresh.process(x), first)
    # the demod AGC setters reach the CW AGC; set_tone belongs to CW alone
    off, (xl2, a2) = dsp.CW(TONE, False, ATT, DEC, FS), cw_single_stages(False)
    sdrpp_amd.check(lib.sdrgpu_demod_agc_set_gain(off._h, 0, 0.25))
    a2.set_gain(0.25)
    assert same(off.process(x), a2.process(real_part(xl2.process(x))))
    gain = np.zeros(1, f32)
    sdrpp_amd.check(lib.sdrgpu_demod_agc_get_gain(off._h, 0, gain.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    assert gain[0] == f32(0.25)
    assert lib.sdrgpu_cw_set_tone(dsp.SSB(0, BW, FS, True, ATT, DEC)._h, 700.0) == -4   # SDRGPU_ESTATE


def cw_stages(S, agc):
    return [dsp.BankXlator(S, rads(TONE)), real_part, dsp.BankAGC(S, *CW_AGC, enabled=agc)]


def test_cw_signal_fires_the_lookahead_often():
    """The condition of the BankCW tests: with max output 1 the look-ahead fires whenever a sample rises above the running
    amplitude -- more than one event per stream and call, counted by the numpy restatement on the AGC's input."""
    A = np.stack(stage_columns(cw_stages(SMAX, True)[:2], cw_input(), CUTS), axis=1)
    ev = cached(("cw_ev",), lambda: ba.agc_events(A, CUTS, *CW_AGC))
    per_stream = np.bincount([k for k, _, _, _ in ev], minlength=SMAX)
    assert len(ev) > SMAX * len(CUTS) and per_stream.min() > len(CUTS), (len(ev), per_stream.min())
    write_report("bank_ssb_parity", {"test": "cw_lookahead_events", "events": len(ev), "calls": len(CUTS),
                                     "per_stream_min": int(per_stream.min()), "per_stream_max": int(per_stream.max())})


@pytest.mark.parametrize("agc", [True, False])
@pytest.mark.parametrize("S", SHAPES)
def test_bank_cw_is_its_stages_and_its_single_stream_handles(S, agc):
    X = cw_input()
    args = (TONE, agc, ATT, DEC, FS)
    for cuts in (WHOLE, CUTS):
        what = f"cw S={S} agc={agc} calls={len(cuts)}"
        ys = in_calls(dsp.BankCW(S, *args), X[:, :S], cuts)
        assert ys[0].dtype == f32
        check_columns(ys, stage_columns(cw_stages(S, agc), X[:, :S], cuts), what + " (stages)")
        refs = column_refs(("cw",) + args, lambda: dsp.CW(*args), X, cuts)
        streams_differ(refs[:S])
        check_columns(ys, refs[:S], what)
    if agc:
        whole, cut = (column_refs(("cw",) + args, lambda: dsp.CW(*args), X, c) for c in (WHOLE, CUTS))
        assert not all(same(a, b) for a, b in zip(whole, cut)), "the calls' ends do not matter here: the cut run would show nothing"


@pytest.mark.parametrize("agc", [True, False])
def test_bank_cw_vs_oracle(agc):
    """AGC on: test_ssb_vs_oracle's bar (the oracle chain alone, its input moved by up to +-4 ulp per sample, moved its
    output by 6e-7 of full scale on the keyed tone: the bar is 16 times that). AGC off: gain min(1, 1e7) = 1 and the clip
    at 1, so the output is the translated real part clipped to +-1: the xlator's bar, 2e-6 max|x|."""
    X = cw_input()[:, :KA_S]
    b = dsp.BankCW(KA_S, TONE, agc, ATT, DEC, FS)
    os_ = [(oracle.Xlator(2 * np.pi * TONE / FS), oracle.AGC(False, *CW_AGC)) for _ in range(KA_S)]
    for _, a in os_:
        a.set_enabled(agc)
    worst, worst_abs, i = 0.0, 0.0, 0
    for n in ORACLE_CALLS:
        y = b.process(X[i:i + n])
        for k in range(KA_S):
            x = col(X[i:i + n], k)
            got, ref = col(y, k), os_[k][1].process(real_part(os_[k][0].process(x)))
            assert got.shape == ref.shape
            err, scale = np.abs(got - ref).max(), max(np.abs(ref).max(), 1e-30)
            tol = 1e-5 * scale + 16 * EPS32 * scale if agc else 2e-6 * np.abs(x).max()
            print(f"cw agc {agc} rows {i}..{i + n} stream {k}: err {err:.3e} tol {tol:.3e}")
            worst, worst_abs = max(worst, err / tol), max(worst_abs, err / scale)
            assert err <= tol, f"cw agc={agc} rows {i}..{i + n}: stream {k} max abs err {err:.3e} > {tol:.3e}"
        i += n
    write_report("bank_ssb_parity", {"test": "cw_vs_oracle", "S": KA_S, "agc": agc, "max_err_over_bound": float(worst),
                                     "max_err_over_scale": float(worst_abs)})


# ------------------------------------------------- 4. channelizer -> BankSSB
def test_channelizer_feeds_bank_ssb_by_device_pointer():
    import torch
    M, NF = 256, 600
    h = dsp.windowed_sinc(16 * M, np.pi / M)                     # tests/test_channelizer.py
    rng = np.random.default_rng(6)
    t = np.arange(NF * M)
    x = 0.003 * (rng.uniform(-1, 1, NF * M) + 1j * rng.uniform(-1, 1, NF * M))
    for k in range(0, M, 3):                                    # a tone in every third channel, keyed per channel
        x += 0.2 * (np.sin(2 * np.pi * (1 + k % 16) * t / (80.0 * M)) > -0.5) * np.exp(2j * np.pi * (k + 0.07) * t / M)
    x = x.astype(np.complex64)
    s = torch.cuda.Stream()
    d_x = torch.from_numpy(x.view(f32)).cuda()
    d_ch = torch.empty(2 * NF * M, dtype=torch.float32, device="cuda")
    d_au = torch.empty(NF * M, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ch = dsp.PolyphaseChannelizer(M, h)
    assert ch.process_dev(d_x.data_ptr(), NF * M, d_ch.data_ptr(), s.cuda_stream) == NF * M
    args = (0, BW, FS, True, ATT, DEC)
    b = dsp.BankSSB(M, *args)
    assert b.process_dev(d_ch.data_ptr(), NF, d_au.data_ptr(), s.cuda_stream) == NF
    s.synchronize()
    C = d_ch.cpu().numpy().view(np.complex64).reshape(NF, M)
    A = d_au.cpu().numpy().reshape(NF, M)
    assert np.abs(C).max() > 0.05
    for k in range(M):
        assert same(col(A, k), dsp.SSB(*args).process(col(C, k))), f"ssb, channel {k}"


# ------------------------------------------------------------ 5. empty calls
@pytest.mark.parametrize("name", ["xlator", "ssb", "cw"])
def test_a_call_of_no_frames_changes_nothing(name):
    S = KA_S
    make, X = {"xlator": (lambda: dsp.BankXlator(S, W1), ssb_input()),
               "ssb": (lambda: dsp.BankSSB(S, 0, BW, FS, True, ATT, DEC), ssb_input()),
               "cw": (lambda: dsp.BankCW(S, TONE, True, ATT, DEC, FS), cw_input())}[name]
    X = X[:, :S]
    assert 0 in CUTS
    with_empty = in_calls(make(), X, CUTS)
    without = in_calls(make(), X, [n for n in CUTS if n])
    for k in range(S):
        assert same(with_empty[k], without[k]), f"{name}: stream {k}"
    b = make()                                                   # also as the first call, and by device pointer with null buffers
    assert b.process(X[:0]).shape == (0, S) and b.process_dev(0, 0, 0) == 0
    assert same(np.stack(in_calls(b, X, WHOLE), axis=1), np.stack(in_calls(make(), X, WHOLE), axis=1))
