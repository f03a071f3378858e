"""Analogue receiver banks on the device (libsdrgpu, HIP): AGC, DC blocker, de-emphasis, squelch, NFM and AM
over S streams per launch in the channelizer's layout x[m, k].

The reference of every bank column is a fresh SINGLE-STREAM handle of the existing block with the same
parameters, fed that column in the same calls. Those blocks are held to the reference by tests/test_loops.py,
tests/test_gpu_parity.py and tests/test_ref_blocks.py; no bar here comes from a bank's own numbers.

Bars:
* DC blocker, de-emphasis, AGC (enabled and the fixed-gain limiter), squelch (outputs and muted[k]) -- every
  column bit-identical to its single-stream handle. The AGC's result depends on where calls end (its clip
  look-ahead spans the call), so a bank run whole is held to handles fed whole columns, and a bank run
  over CUTS to handles fed the same cuts.
* BankFM (4 filter combinations), BankAM (3 AGC modes) -- bit-identical to their bank stages run one after
  another; within 1e-3 of oracle.FM (test_fm_nfm_vs_oracle's bar) and within fir_atol(lpf, [2 max|y|]) of
  oracle.AM(precise=True) (test_am_vs_oracle's bar and burst).
* Known answer at S = 65: the strongest bin of every BankFM column is that stream's tone.
* Channelizer -> BankSquelch -> BankFM and -> BankAM by device pointer.
* Shapes, cuts and the rule that streams differ: tests/test_banks.py.
The parity summary goes to bank_audio_parity.jsonl through write_report.
"""
import numpy as np
import pytest

import oracle
import sdrpp_amd
from sdrpp_amd import dsp
from _util import fir_atol, write_report
from _restated import same
from test_banks import (FRAMES, SHAPES, SMAX, TILE, CUTS, cached, noise_bank, single_columns, run_whole, run_cuts, whole_and_cut,
                        check_columns, streams_differ)
import _bank_audio as ba

pytestmark = pytest.mark.gpu

f32 = np.float32
FS = 48000.0
AGC_ARGS = ba.AGC_ARGS
assert (FRAMES, SMAX, TILE) == (ba.FRAMES, ba.SMAX, ba.TILE)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"


def col(X, k):
    return np.ascontiguousarray(X[:, k])


def cut_columns(key, make_single, X, cuts=CUTS):
    """The reference of a run in calls, once per configuration: column k through a fresh handle fed the same cuts."""
    def make():
        refs = []
        for k in range(X.shape[1]):
            h, x, i, parts = make_single(), col(X, k), 0, []
            for n in cuts:
                parts.append(h.process(x[i:i + n]))
                i += n
            refs.append(np.concatenate(parts))
        return refs
    return cached(("cutref",) + key, make)


def offset_bank(cplx):
    """noise_bank plus a DC offset per stream"""
    def make():
        X = noise_bank(cplx).copy()
        for k in range(SMAX):
            X[:, k] += (0.3 + 0.2j) * (1 + k % 3) if cplx else f32(0.25 * (1 + k % 3))
        return X
    return cached(("offset", cplx), make)


# --------------------------------------- 1. DC blocker, de-emphasis: bit-identical
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("S", SHAPES)
def test_dc_blocker_columns(S, cplx):
    X, rate = offset_bank(cplx), 10.0 / FS
    refs = single_columns(("dcb", cplx), lambda: dsp.DCBlocker(rate, cplx), X)
    ys, _ = whole_and_cut(lambda: dsp.BankDCBlocker(S, rate, complex_data=cplx), X[:, :S], f"dc_blocker S={S} cplx={cplx}")
    streams_differ(refs[:S])
    check_columns(ys, refs[:S], f"dc_blocker S={S} cplx={cplx}")


@pytest.mark.parametrize("S", SHAPES)
def test_deemphasis_columns(S):
    X = offset_bank(False)
    refs = single_columns(("deemp",), lambda: dsp.Deemphasis(50e-6, FS), X)
    ys, _ = whole_and_cut(lambda: dsp.BankDeemphasis(S, 50e-6, FS), X[:, :S], f"deemphasis S={S}")
    streams_differ(refs[:S])
    check_columns(ys, refs[:S], f"deemphasis S={S}")


# ------------------------------------------------------------------- 2. AGC
def agc_input(cplx):
    return cached(("agc_in", cplx), lambda: ba.agc_bank(cplx))


def agc_event_list(cplx, cuts):
    return cached(("agc_ev", cplx, tuple(cuts)), lambda: ba.agc_events(agc_input(cplx), cuts, *AGC_ARGS))


@pytest.mark.parametrize("cplx", [False, True])
def test_agc_signal_fires_the_lookahead_where_it_matters(cplx):
    """The condition of the AGC tests, counted by the numpy restatement: over the bank, look-ahead events at tile rows
    0 and 31, in a tile that is not its call's last, in a call's last tile and in a call's last row."""
    ev = agc_event_list(cplx, [FRAMES]) + agc_event_list(cplx, CUTS)
    tile_rows = {r % TILE for _, _, r, _ in ev}
    assert 0 in tile_rows and TILE - 1 in tile_rows, sorted(tile_rows)
    assert any(r // TILE < (n - 1) // TILE for _, _, r, n in ev), "no event in a tile that is not the call's last"
    assert any(r // TILE == (n - 1) // TILE for _, _, r, n in ev), "no event in the last tile of a call"
    assert any(r == n - 1 for _, _, r, n in ev), "no event in a call's last row"
    per_stream = np.bincount([k for k, _, _, _ in ev], minlength=SMAX)
    write_report("bank_audio_parity", {"test": "agc_lookahead_events", "complex": cplx, "events": len(ev),
                                       "per_stream_min": int(per_stream.min()), "per_stream_max": int(per_stream.max()),
                                       "tile_rows": sorted(int(r) for r in tile_rows)})


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("S", SHAPES)
def test_agc_enabled_columns(S, cplx):
    X = agc_input(cplx)
    for cuts in ([FRAMES], CUTS):
        per_stream = np.bincount([k for k, _, _, _ in agc_event_list(cplx, cuts)], minlength=SMAX)
        assert per_stream[:S].min() >= 1, "a stream without a look-ahead event"
    make = lambda: dsp.BankAGC(S, *AGC_ARGS, complex_data=cplx)
    single = lambda: dsp.AGC(*AGC_ARGS, complex_data=cplx)
    what = f"agc S={S} cplx={cplx}"
    whole = single_columns(("agc_on", cplx), single, X)
    streams_differ(whole[:S])
    check_columns(run_whole(make(), X[:, :S])[0], whole[:S], what + " whole")
    cut = cut_columns(("agc_on", cplx), single, X)
    assert not all(same(a, b) for a, b in zip(whole, cut)), "the calls' ends do not matter here: the cut run would show nothing"
    check_columns(run_cuts(make(), X[:, :S]), cut[:S], what + " cut")


def limiter(cplx):
    a = dsp.AGC(1.0, AGC_ARGS[1], AGC_ARGS[2], 10e6, 10.0, 3.5, complex_data=cplx)
    a.set_enabled(False)
    a.set_gain(3.5)
    return a


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("S", SHAPES)
def test_agc_disabled_columns_and_set_gain(S, cplx):
    X = agc_input(cplx)
    make = lambda: dsp.BankAGC(S, 1.0, AGC_ARGS[1], AGC_ARGS[2], 10e6, 10.0, 3.5, complex_data=cplx, enabled=False)
    refs = single_columns(("agc_off", cplx), lambda: limiter(cplx), X)
    assert any(np.abs(r).max() > 9.99 for r in refs) and np.abs(refs[0][:100]).max() < 9.0, "the limiter never limits, or always"
    ys, _ = whole_and_cut(make, X[:, :S], f"agc off S={S} cplx={cplx}")
    streams_differ(refs[:S])
    check_columns(ys, refs[:S], f"agc off S={S} cplx={cplx}")

    def regained():                                              # set_gain(2.0) between two calls
        out = []
        for k in range(SMAX):
            a = limiter(cplx)
            first = a.process(col(X, k)[:2000])
            a.set_gain(2.0)
            out.append(np.concatenate([first, a.process(col(X, k)[2000:])]))
        return out
    refs2 = cached(("agc_regain", cplx), regained)
    assert not same(refs2[0], refs[0])
    b = make()
    first, _ = run_whole(b, X[:2000, :S])
    b.set_gain(2.0)
    second, _ = run_whole(b, X[2000:, :S])
    check_columns([np.concatenate(p) for p in zip(first, second)], refs2[:S], f"agc off set_gain S={S} cplx={cplx}")


# --------------------------------------------------------------- 3. squelch
def squelch_reference():
    """Per call: the handles' outputs (n, SMAX) and is_muted() [SMAX]"""
    def make():
        calls = ba.squelch_calls()
        hs = [dsp.Squelch(ba.SQ_LEVEL) for _ in range(SMAX)]
        outs, muted = [], []
        for x in calls:
            outs.append(np.stack([h.process(col(x, k)) for k, h in enumerate(hs)], axis=1))
            muted.append(np.array([h.is_muted() for h in hs], np.int32))
        return calls, outs, np.array(muted)
    return cached(("squelch_ref",), make)


def test_squelch_schedule_is_what_it_claims():
    calls, _, muted = squelch_reference()
    sizes = [len(x) for x in calls]
    assert sizes.count(480) >= 30 and {0, 1, 31, 33} <= set(sizes)
    for c, x in enumerate(calls):                               # every decision is a dB away from both thresholds
        if len(x):
            db = 20 * np.log10(np.abs(x.astype(np.complex128)).mean(axis=0))
            assert np.all(np.minimum(np.abs(db - ba.SQ_LEVEL), np.abs(db - (ba.SQ_LEVEL - 1))) >= 1.0), f"call {c}"
    live = [c for c, n in enumerate(sizes) if n]                 # (an empty call decides nothing)
    m = muted[live]
    assert len({tuple(m[:, k]) for k in range(SMAX)}) >= 10, "streams mute and unmute at the same calls"
    # stream 1: quiet at calls 3, 4 -> muted at 3, the count set at 4; calls 5.. are loud: exactly 10 of them unmute
    loud1 = [c for c in live if c >= 5]
    assert muted[3, 1] and muted[loud1[8], 1] and not muted[loud1[9], 1]
    # stream 2: the same with call 10 quiet: the count restarts there and runs 10 loud calls from call 11
    loud2 = [c for c in live if c >= 11]
    assert muted[loud1[9], 2] and muted[loud2[8], 2] and not muted[loud2[9], 2]
    assert not muted[:, 0].any()


@pytest.mark.parametrize("S", SHAPES)
def test_squelch_columns_and_muted(S):
    calls, outs, muted = squelch_reference()
    b = dsp.BankSquelch(S, ba.SQ_LEVEL)
    for c, x in enumerate(calls):
        y = b.process(x[:, :S])
        assert y.shape == (len(x), S)
        for k in range(S):
            assert same(col(y, k), col(outs[c], k)), f"squelch S={S}: call {c} ({len(x)} rows), stream {k}"
        m = b.muted
        assert m.dtype == np.int32 and list(m) == list(muted[c, :S]), f"squelch S={S}: muted after call {c}"


# ------------------------------------------- 4. composites are their stages
def run_stage_list(stages, X, cuts):
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


def fm_taps(bw, lp, hp):
    if lp and hp:
        return dsp.band_pass(300.0, bw / 2.0, 100.0, FS)
    return dsp.high_pass(300.0, 100.0, FS) if hp else dsp.low_pass(bw / 2.0, (bw / 2.0) * 0.1, FS)


def fm_stages(S, bw, lp, hp):
    st = [dsp.BankQuadrature(S, 2 * np.pi * (bw / 2.0) / FS)]
    return st + ([dsp.BankFIR(S, fm_taps(bw, lp, hp), complex_data=False)] if lp or hp else [])


AM_ARGS = (10000.0, AGC_ARGS[1], AGC_ARGS[2], 10.0 / FS, FS)     # bandwidth, attack, decay, dcBlockRate, samplerate


def am_stages(S, mode):
    agc = lambda cplx, on: dsp.BankAGC(S, *AGC_ARGS, complex_data=cplx, enabled=on)
    return ([agc(True, True)] if mode == 1 else []) + [ba.amplitude, dsp.BankDCBlocker(S, AM_ARGS[3])] + \
           ([agc(False, mode == 2)] if mode != 1 else []) + [dsp.BankFIR(S, dsp.low_pass(5000.0, 500.0, FS), complex_data=False)]


@pytest.mark.parametrize("lp,hp", [(True, False), (False, True), (True, True), (False, False)])
@pytest.mark.parametrize("S", SHAPES)
def test_bank_fm_is_its_stages(S, lp, hp):
    X = noise_bank(True)[:, :S]
    ys, _ = whole_and_cut(lambda: dsp.BankFM(S, FS, 12500.0, lp, hp), X, f"fm S={S} lp={lp} hp={hp}")
    assert ys[0].dtype == f32
    check_columns(ys, run_stage_list(fm_stages(S, 12500.0, lp, hp), X, [FRAMES]), f"fm S={S} lp={lp} hp={hp}")


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("S", SHAPES)
def test_bank_am_is_its_stages(S, mode):
    X = agc_input(True)[:, :S]
    ys, _ = run_whole(dsp.BankAM(S, mode, *AM_ARGS), X)
    assert ys[0].dtype == f32
    check_columns(ys, run_stage_list(am_stages(S, mode), X, [FRAMES]), f"am S={S} mode={mode} whole")
    check_columns(run_cuts(dsp.BankAM(S, mode, *AM_ARGS), X), run_stage_list(am_stages(S, mode), X, CUTS), f"am S={S} mode={mode} cut")


def test_bank_am_set_agc_gain_reaches_the_audio_agc():
    S, X = 65, agc_input(True)[:, :65]
    b, st = dsp.BankAM(S, 0, *AM_ARGS), am_stages(S, 0)
    b.set_agc_gain(2.0)
    st[2].set_gain(2.0)
    y = b.process(X)
    zs = run_stage_list(st, X, [FRAMES])
    check_columns([col(y, k) for k in range(S)], zs, "am set_agc_gain")
    assert not same(col(y, 0), col(dsp.BankAM(S, 0, *AM_ARGS).process(X), 0)), "the gain does not matter here"


# ------------------------------------------ 5. against the project's bars
KA_S = 65


@pytest.mark.parametrize("lp,hp", [(True, False), (False, True), (True, True), (False, False)])
def test_bank_fm_vs_oracle(lp, hp):
    X = noise_bank(True)[:, :KA_S]
    y = dsp.BankFM(KA_S, 48000, 12500, lp, hp).process(X)
    worst = 0.0
    for k in range(KA_S):
        err = np.abs(col(y, k) - oracle.FM(48000, 12500, lp, hp).process(col(X, k))).max()
        worst = max(worst, err)
        assert err < 1e-3, f"fm lp={lp} hp={hp}: stream {k} max abs err {err:.3e}"
    write_report("bank_audio_parity", {"test": "fm_vs_oracle", "S": KA_S, "low_pass": lp, "high_pass": hp, "max_err": float(worst),
                                       "max_err_over_bound": float(worst / 1e-3)})


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_bank_am_vs_oracle(mode):
    n, calls = 4200, [(0, 480), (480, 3000), (3000, 4200)]
    X = cached(("am_burst",), lambda: ba.am_burst_bank(KA_S, n, FS))
    ev = cached(("am_burst_ev",), lambda: ba.agc_events(X, [e - s for s, e in calls], *AGC_ARGS))
    burst = {k for k, c, r, _ in ev if c == 1 and 2000 - 480 <= r < 2100 - 480}
    assert burst == set(range(KA_S)), "the burst does not fire every stream's carrier AGC look-ahead"
    args = (mode,) + AM_ARGS
    b, os_ = dsp.BankAM(KA_S, *args), [oracle.AM(*args, precise=True) for _ in range(KA_S)]
    lpf, worst = oracle.low_pass(5000.0, 500.0, FS), 0.0
    for s, e in calls:
        y = b.process(X[s:e])
        for k in range(KA_S):
            ref = os_[k].process(col(X[s:e], k))
            err, tol = np.abs(col(y, k) - ref).max(), fir_atol(lpf, np.array([np.abs(ref).max() * 2]))
            worst = max(worst, err / tol)
            assert err <= tol, f"am mode {mode} rows {s}..{e}: stream {k} max abs err {err:.3e} > {tol:.3e}"
    write_report("bank_audio_parity", {"test": "am_vs_oracle", "S": KA_S, "mode": mode, "max_err_over_bound": float(worst)})


def test_fm_tone_known_answer_per_stream():
    n = 4800                                                    # 10 Hz bins: tone 300 + 20 k Hz is bin 30 + 2 k
    X = ba.fm_tone_bank(KA_S, n, FS, lambda k: 300 + 20 * k, 2000.0)
    y = dsp.BankFM(KA_S, FS, 12500.0, True, False).process(X)
    peaks = [int(np.argmax(np.abs(np.fft.rfft(col(y, k).astype(np.float64)))[1:]) + 1) for k in range(KA_S)]
    assert peaks == [30 + 2 * k for k in range(KA_S)]


# ------------------------------------------- 6. channelizer -> banks on the device
def test_channelizer_feeds_audio_banks_by_device_pointer():
    import torch
    M, NF = 256, 600
    h = dsp.windowed_sinc(16 * M, np.pi / M)                     # tests/test_channelizer.py
    rng = np.random.default_rng(6)
    t = np.arange(NF * M)
    x = 0.003 * (rng.uniform(-1, 1, NF * M) + 1j * rng.uniform(-1, 1, NF * M))
    for k in range(0, M, 3):                                    # a carrier in every third channel, AM by a tone per channel
        x += 0.2 * (1 + 0.5 * np.sin(2 * np.pi * (1 + k % 16) * t / (80.0 * M))) * np.exp(2j * np.pi * (k + 0.1) * t / M)
    x = x.astype(np.complex64)
    s = torch.cuda.Stream()
    d_x = torch.from_numpy(x.view(f32)).cuda()
    d_ch = torch.empty(2 * NF * M, dtype=torch.float32, device="cuda")
    d_sq = torch.empty(2 * NF * M, dtype=torch.float32, device="cuda")
    d_fm = torch.empty(NF * M, dtype=torch.float32, device="cuda")
    d_am = torch.empty(NF * M, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ch = dsp.PolyphaseChannelizer(M, h)
    assert ch.process_dev(d_x.data_ptr(), NF * M, d_ch.data_ptr(), s.cuda_stream) == NF * M
    s.synchronize()
    C = d_ch.cpu().numpy().view(np.complex64).reshape(NF, M)
    # the squelch level: the middle of the widest gap between the channels' levels (carriers above, noise below)
    db = np.sort(20 * np.log10(np.abs(C.astype(np.complex128)).mean(axis=0)))
    g = int(np.argmax(np.diff(db)))
    level = float(0.5 * (db[g] + db[g + 1]) + 0.5)
    assert db[g + 1] - level >= 1.0 and (level - 1.0) - db[g] >= 1.0, "a channel's level within 1 dB of a threshold"
    sq, fm, am = dsp.BankSquelch(M, level), dsp.BankFM(M, FS, 12500.0, True, False), dsp.BankAM(M, 1, *AM_ARGS)
    assert sq.process_dev(d_ch.data_ptr(), NF, d_sq.data_ptr(), s.cuda_stream) == NF
    assert fm.process_dev(d_sq.data_ptr(), NF, d_fm.data_ptr(), s.cuda_stream) == NF
    assert am.process_dev(d_ch.data_ptr(), NF, d_am.data_ptr(), s.cuda_stream) == NF
    s.synchronize()
    Q = d_sq.cpu().numpy().view(np.complex64).reshape(NF, M)
    F, A = d_fm.cpu().numpy().reshape(NF, M), d_am.cpu().numpy().reshape(NF, M)
    muted = sq.muted
    assert 0 < muted.sum() < M
    taps, lpf = fm_taps(12500.0, True, False), dsp.low_pass(5000.0, 500.0, FS)
    corr = lambda v, tp: np.convolve(v.astype(np.float64), tp.astype(np.float64)[::-1])[:NF]
    for k in range(M):
        one = dsp.Squelch(level)
        assert same(col(Q, k), one.process(col(C, k))) and one.is_muted() == bool(muted[k]), f"squelch, channel {k}"
        q = dsp.Quadrature(2 * np.pi * 6250.0 / FS).process(col(Q, k))
        assert np.abs(col(F, k) - corr(q, taps)).max() <= fir_atol(taps, q), f"fm, channel {k}"
        pre = dsp.DCBlocker(AM_ARGS[3]).process(ba.amplitude(dsp.AGC(*AGC_ARGS, complex_data=True).process(col(C, k))))
        assert np.abs(col(A, k) - corr(pre, lpf)).max() <= fir_atol(lpf, pre), f"am, channel {k}"


# -------------------------------------------------------------------- 7. reset
def _loud_then_quiet():
    loud = 10.0 ** ((ba.SQ_LEVEL + 6) / 20.0) * np.exp(2j * np.pi * np.random.default_rng(3).uniform(0, 1, (960, 65)))
    loud[480:] *= 10.0 ** (-14 / 20.0)                          # rows 0..479 loud, 480..959 quiet
    return loud.astype(np.complex64)


@pytest.mark.parametrize("name", ["agc", "agc_complex", "dc_blocker", "dc_blocker_complex", "deemphasis", "squelch", "fm", "am"])
def test_reset_reproduces_the_first_run(name):
    S = 65
    make, X = {
        "agc": (lambda: dsp.BankAGC(S, *AGC_ARGS), agc_input(False)),
        "agc_complex": (lambda: dsp.BankAGC(S, *AGC_ARGS, complex_data=True), agc_input(True)),
        "dc_blocker": (lambda: dsp.BankDCBlocker(S, 10.0 / FS), offset_bank(False)),
        "dc_blocker_complex": (lambda: dsp.BankDCBlocker(S, 10.0 / FS, complex_data=True), offset_bank(True)),
        "deemphasis": (lambda: dsp.BankDeemphasis(S, 50e-6, FS), offset_bank(False)),
        "squelch": (lambda: dsp.BankSquelch(S, ba.SQ_LEVEL), _loud_then_quiet()),
        "fm": (lambda: dsp.BankFM(S, FS, 12500.0), noise_bank(True)),
        "am": (lambda: dsp.BankAM(S, 2, *AM_ARGS), agc_input(True)),
    }[name]
    X = X[:960, :S]
    b = make()
    run = lambda: np.concatenate([b.process(X[:480]), b.process(X[480:])])   # (squelch: a loud call, then a quiet one)
    first = run()
    b.reset()
    if name == "am":
        # AM::reset() (am.h:104-112) resets the AGCs and the DC blocker and leaves the low-pass filter's history, as
        # tests/test_ref_demod.py pins to the reference: the run after it agrees with the first one from the row on
        # at which the filter holds this run's rows only, and not before
        H = len(dsp.low_pass(AM_ARGS[0] / 2.0, (AM_ARGS[0] / 2.0) * 0.1, FS)) - 1
        again = run()
        assert 0 < H < 480 and same(again[H:], first[H:]) and not same(again[:H], first[:H])
    else:
        assert same(run(), first)
    assert not same(run(), first), "the state does not matter here: the check would show nothing"
