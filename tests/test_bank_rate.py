"""Rate-changing banks on the device (libsdrgpu, HIP): decimating FIR, polyphase resampler, power decimator and
rational resampler over S streams in the channelizer's layout x[m, k].

Bars, all from the project:
* Decimating FIR -- bit-identical to rows [0 :: D] of BankFIR with the same taps; every column within
  fir_atol(taps, x_k) of oracle.FIR(taps, D), with equal lengths.
* Polyphase -- every column within the largest fir_atol(phase taps, x_k) over the phases of
  oracle.PolyphaseResampler, with equal lengths; (1, D) bit-identical to the decimating FIR bank.
* Impulses -- the outputs are taps (of the row's phase), exactly, and zero outside them.
* Power decimator, rational resampler -- bit-identical to their stages run as separate banks; within
  test_power_decimator's 2e-5 / test_rational_resampler's 5e-5 of the oracle on unscaled _util.iq noise.
* Every configuration: the tiled kernel and the direct kernel give the same bits; a bank run whole and a
  fresh one over cuts give the same bits; before every call out_rows(frames) is the rows the call returns,
  after it counts are all that number.
* Shapes: S in {1, 63, 64, 65, 130}, 4200 rows; stream k's data from its own seed and scale, columns
  compared one by one. The cuts: one row, an empty call, runs of calls shorter than the decimation (several
  calls in a row without an output row), a call shorter than the history, the history edge, the tiled
  kernel's input-row span edge, 1024.
The parity summary goes to bank_rate_parity.jsonl through write_report.
"""
import contextlib
import os

import numpy as np
import pytest

import oracle
import sdrpp_amd
from sdrpp_amd import dsp
from _util import fir_atol, iq, write_report
from _restated import same

pytestmark = pytest.mark.gpu

f32 = np.float32
FRAMES = 4200
SHAPES = [1, 63, 64, 65, 130]
SMAX = max(SHAPES)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"


# ------------------------------------------------------------------- inputs
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def noise_bank(cplx):
    """(FRAMES, SMAX): stream k is uniform noise from default_rng(100 + k) scaled by 0.25 + 0.25 (k mod 8)
    (the streams of tests/test_banks.py)."""
    def make():
        X = np.empty((FRAMES, SMAX), np.complex64 if cplx else f32)
        for k in range(SMAX):
            rng = np.random.default_rng(100 + k)
            x = rng.uniform(-1, 1, FRAMES).astype(f32)
            if cplx:
                x = (x + 1j * rng.uniform(-1, 1, FRAMES).astype(f32)).astype(np.complex64)
            X[:, k] = x * f32(0.25 + 0.25 * (k % 8))
        return X
    return cached(("noise", cplx), make)


def iq_bank(cplx):
    """(FRAMES, SMAX): stream k is _util.iq(default_rng(500 + k)), unscaled (real: its real part)."""
    def make():
        X = np.stack([iq(np.random.default_rng(500 + k), FRAMES) for k in range(SMAX)], axis=1)
        return np.ascontiguousarray(X if cplx else X.real)
    return cached(("iq", cplx), make)


def oracle_columns(key, make, X):
    """The reference, once per configuration: column k of X through a fresh oracle object."""
    return cached(("oracle",) + key, lambda: [make().process(np.ascontiguousarray(X[:, k])) for k in range(X.shape[1])])


# -------------------------------------------------------- the kernel's two forms
TILE_LDS, TILE_RMIN, TILE_RMAX = 64 * 1024, 4, 64                 # bank_rate_kernels.h RATE_LDS, RATE_RMIN, RATE_RMAX


def tile_rows(cplx, interp, decim, tpp):
    """BankRate::rate_tile_rows (bank.hip): output rows per tile of the tiled kernel, 0 where no tile fits."""
    room = TILE_LDS // (64 * (8 if cplx else 4)) - tpp
    if room < 0:
        return 0
    r = min(room * interp // decim + 1, TILE_RMAX)
    return r if r >= TILE_RMIN else 0


def tile_span(cplx, interp, decim, ntaps):
    """the input rows that one tile's output rows consume (32 where the configuration has no tile), for the largest
    tile and for the tile of 8 rows that a call with few rows takes (BankRate::run)"""
    r = tile_rows(cplx, interp, decim, -(-ntaps // interp))
    return (max(r * decim // interp, 2), max(min(r, 8) * decim // interp, 2)) if r else (32, 32)


@contextlib.contextmanager
def form(tiled):
    """banks created inside run the tiled (where the tile fits) or the direct kernel: the knob is read at creation"""
    keys = ("SDRGPU_TUNING", "SDRGPU_BANK_RATE_TILED")
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update(SDRGPU_TUNING="1", SDRGPU_BANK_RATE_TILED="1" if tiled else "0")
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------ running banks
def cuts_for(hist, span):
    """calls: one row, an empty one, single rows and pairs (shorter than a decimation of 7 or 8: runs of calls
    without an output row; for a decimation of 2 every other single row has none), half the history, the history
    edge, the span edge, 1024, the rest"""
    c = [1, 0, 1, 1, 1, 2, 1, 1, 1, 3, 1, 0, 0, 1]
    c += [max(hist // 2, 1)] + [n for n in (hist - 1, hist, hist + 1) if n > 0]
    for n in sorted(set(span)):
        c += [n - 1, n, n + 1]
    c += [1024]
    assert sum(c) < FRAMES
    return c + [FRAMES - sum(c)]


def call(bank, X):
    want = bank.out_rows(len(X))
    y = bank.process(X)
    assert len(y) == want, f"out_rows({len(X)}) = {want}, the call wrote {len(y)} rows"
    c = bank.counts
    assert c.dtype == np.int32 and c.shape == (bank.streams,) and np.all(c == len(y)), f"counts {c} after {len(y)} rows"
    return y.copy()


def run_cuts(bank, X, cuts):
    parts, i, empty = [], 0, 0
    for n in cuts:
        parts.append(call(bank, X[i:i + n]))
        empty += n > 0 and len(parts[-1]) == 0
        i += n
    assert i == len(X)
    return np.concatenate(parts), empty


def all_forms(make, X, cuts, what, zero_row_calls=0):
    """the bank whole and over cuts, tiled and direct: one answer"""
    outs = []
    for tiled in (True, False):
        with form(tiled):
            y = call(make(), X)
            z, empty = run_cuts(make(), X, cuts)
        assert empty >= zero_row_calls, f"{what}: {empty} calls with rows in and none out, the cuts should make {zero_row_calls}"
        assert same(y, z), f"{what}: {'tiled' if tiled else 'direct'} in calls differs from one call"
        outs.append(y)
    assert same(outs[0], outs[1]), f"{what}: the tiled and the direct kernel differ"
    return outs[0]


def run_stages(stages, X):
    for b in stages:
        X = call(b, X)
    return X


def check_columns(Y, refs, tol, what):
    """every column within its bound of its reference, with equal lengths; returns the worst err / bound"""
    worst = 0.0
    for k in range(Y.shape[1]):
        assert len(refs[k]) == Y.shape[0], f"{what}: stream {k} has {Y.shape[0]} rows, the oracle {len(refs[k])}"
        err, bound = np.abs(Y[:, k].astype(np.complex128) - refs[k]).max(), tol(k)
        worst = max(worst, err / bound)
        assert err <= bound, f"{what}: stream {k} max abs err {err:.3e} > {bound:.3e}"
    return worst


def streams_differ(Y):
    assert Y.shape[1] < 2 or not any(same(Y[:, 0], Y[:, k]) for k in range(1, Y.shape[1])), "streams with equal outputs show nothing"


# ---------------------------------------------------------- 1. decimating FIR
DFIR_TAPS = {"one": lambda: np.array([0.75], f32),
             "ramp8": lambda: (np.arange(1, 9) / 8.0).astype(f32) * np.array([1, -1, 1, 1, -1, 1, -1, -1], f32),
             "plan69": lambda: dsp.decim_plan(2)[0][1]}


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("name", sorted(DFIR_TAPS))
@pytest.mark.parametrize("D", [2, 7, 8])
@pytest.mark.parametrize("S", SHAPES)
def test_decimating_fir(S, D, name, cplx):
    taps = DFIR_TAPS[name]()
    T = len(taps)
    assert T == {"one": 1, "ramp8": 8, "plan69": 69}[name]
    X = noise_bank(cplx)
    what = f"decimating fir {name} / {D} S={S} cplx={cplx}"
    cuts = cuts_for(T - 1, tile_span(cplx, 1, D, T))
    Y = all_forms(lambda: dsp.BankDecimatingFIR(S, taps, D, complex_data=cplx), X[:, :S], cuts, what, zero_row_calls=3)
    assert Y.shape == (-(-FRAMES // D), S)
    streams_differ(Y)
    full = cached(("bankfir", name, cplx), lambda: dsp.BankFIR(SMAX, taps, complex_data=cplx).process(X).copy())
    assert same(Y, np.ascontiguousarray(full[::D, :S])), f"{what}: differs from rows [0::{D}] of BankFIR"
    refs = oracle_columns(("fir", name, D, cplx), lambda: oracle.FIR(taps, D, complex_data=cplx), X)
    worst = check_columns(Y, refs, lambda k: fir_atol(taps, X[:, k]), what)
    write_report("bank_rate_parity", {"test": "decimating_fir", "taps": name, "decim": D, "S": S, "frames": FRAMES, "complex": cplx,
                                      "max_err_over_bound": worst})


# --------------------------------------------------------------- 2. polyphase
def poly_taps(interp, decim):                                   # tests/test_gpu_parity.py test_polyphase
    return dsp.low_pass(0.4 / max(interp, decim), 0.05 / max(interp, decim), 1.0) * interp


POLY = {"4/5": (4, 5, lambda: poly_taps(4, 5)), "3/2": (3, 2, lambda: poly_taps(3, 2)), "1/7": (1, 7, lambda: poly_taps(1, 7)),
        "5/4": (5, 4, lambda: poly_taps(5, 4)),
        "3/2 of 8 taps": (3, 2, DFIR_TAPS["ramp8"]),             # ntaps % interp != 0
        "16/5 of 5 taps": (16, 5, lambda: np.array([0.5, -1.0, 0.25, 2.0, -0.125], f32))}   # ntaps < interp


def phase_bank(taps, interp):
    """multirate/polyphase_bank.h:15-47: phases[P - 1 - (i % P)][i / P] = taps[i], zero-padded"""
    tpp = -(-len(taps) // interp)
    b = np.zeros((interp, tpp), f32)
    for i, t in enumerate(taps):
        b[interp - 1 - i % interp, i // interp] = t
    return b


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("name", sorted(POLY))
@pytest.mark.parametrize("S", SHAPES)
def test_polyphase(S, name, cplx):
    interp, decim, mk = POLY[name]
    taps = np.ascontiguousarray(mk(), f32)
    bank = phase_bank(taps, interp)
    if name == "3/2 of 8 taps":
        assert len(taps) > interp and len(taps) % interp != 0
    if name == "16/5 of 5 taps":
        assert len(taps) < interp
    X = noise_bank(cplx)
    what = f"polyphase {name} S={S} cplx={cplx}"
    cuts = cuts_for(bank.shape[1] - 1, tile_span(cplx, interp, decim, len(taps)))
    Y = all_forms(lambda: dsp.BankPolyphaseResampler(S, interp, decim, taps, complex_data=cplx), X[:, :S], cuts, what,
                  zero_row_calls=3 if decim >= 7 * interp else 0)
    assert Y.shape == (-(-FRAMES * interp // decim), S)
    streams_differ(Y)
    refs = oracle_columns(("poly", name, cplx), lambda: oracle.PolyphaseResampler(interp, decim, taps, complex_data=cplx), X)
    worst = check_columns(Y, refs, lambda k: max(fir_atol(p, X[:, k]) for p in bank), what)
    if interp == 1:
        Z = call(dsp.BankDecimatingFIR(S, taps, decim, complex_data=cplx), X[:, :S])
        assert same(Y, Z), f"{what}: differs from the decimating FIR bank"
    write_report("bank_rate_parity", {"test": "polyphase", "ratio": name, "ntaps": len(taps), "S": S, "frames": FRAMES, "complex": cplx,
                                      "max_err_over_bound": worst})


# ---------------------------------------------------------------- 3. impulses
def impulses(S, cplx, rows=256):
    """stream k: a unit impulse at row k mod 11"""
    X = np.zeros((rows, S), np.complex64 if cplx else f32)
    for k in range(S):
        X[k % 11, k] = 1
    return X


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("name,D", [("ramp8", 2), ("plan69", 7), ("one", 8), ("plan69", 2)])
def test_decimating_fir_impulse_response(name, D, cplx):
    S, taps = 65, DFIR_TAPS[name]()
    T = len(taps)
    X = impulses(S, cplx)
    for tiled in (True, False):
        with form(tiled):
            Y = call(dsp.BankDecimatingFIR(S, taps, D, complex_data=cplx), X)
        hit = 0
        for k in range(S):
            r = k % 11
            idx = r + T - 1 - np.arange(len(Y)) * D              # out[j] = sum_t buf[j D + t] taps[t], the impulse at buf[r + T - 1]
            want = np.where((idx >= 0) & (idx < T), taps[np.clip(idx, 0, T - 1)], f32(0)).astype(X.dtype)
            hit += np.count_nonzero(want) > 0                    # (one tap / 8: only the impulses at rows 0 and 8 are sampled)
            assert same(Y[:, k] + 0, want + 0), f"stream {k} tiled={tiled}"   # (+ 0: -0.0 and 0.0 are the same answer)
        assert hit >= 2 * (S // 11)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("name", sorted(POLY))
def test_polyphase_impulse_response(name, cplx):
    S = 65
    interp, decim, mk = POLY[name]
    taps = np.ascontiguousarray(mk(), f32)
    bank = phase_bank(taps, interp)
    tpp = bank.shape[1]
    X = impulses(S, cplx, rows=1024)
    for tiled in (True, False):
        with form(tiled):
            Y = call(dsp.BankPolyphaseResampler(S, interp, decim, taps, complex_data=cplx), X)
        off, ph = np.divmod(np.arange(len(Y)) * decim, interp)
        for k in range(S):
            idx = k % 11 + tpp - 1 - off                         # the impulse at work row r + tpp - 1
            want = np.where((idx >= 0) & (idx < tpp), bank[ph, np.clip(idx, 0, tpp - 1)], f32(0)).astype(X.dtype)
            assert np.count_nonzero(want) > 0
            assert same(Y[:, k] + 0, want + 0), f"stream {k} tiled={tiled}"


# --------------------------------------------------------- 4. power decimator
def chain_cuts(stages, cplx):
    """the cuts of the stage with the longest history, at the chain's input"""
    hist = max(-(-len(t) // i) - 1 for i, d, t in stages)
    i, d, t = stages[0]
    return cuts_for(hist, tile_span(cplx, i, d, len(t)))


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ratio", [2, 4, 8])
@pytest.mark.parametrize("S", SHAPES)
def test_power_decimator(S, ratio, cplx):
    plan = dsp.decim_plan(ratio)
    X = iq_bank(cplx)
    what = f"power decimator {ratio} S={S} cplx={cplx}"
    cuts = chain_cuts([(1, d, t) for d, t in plan], cplx)
    Y = all_forms(lambda: dsp.BankPowerDecimator(S, ratio, complex_data=cplx), X[:, :S], cuts, what, zero_row_calls=3)
    assert Y.shape == ({2: 2100, 4: 1050, 8: 525}[ratio], S)
    streams_differ(Y)
    Z = run_stages([dsp.BankDecimatingFIR(S, t, d, complex_data=cplx) for d, t in plan], X[:, :S])
    assert same(Y, Z), f"{what}: differs from its stages run as separate banks"
    refs = oracle_columns(("pdec", ratio, cplx), lambda: oracle.PowerDecimator(ratio, complex_data=cplx), X)
    worst = check_columns(Y, refs, lambda k: 2e-5, what)
    write_report("bank_rate_parity", {"test": "power_decimator", "ratio": ratio, "S": S, "frames": FRAMES, "complex": cplx,
                                      "max_abs_err": worst * 2e-5, "bound": 2e-5})


def test_power_decimator_of_one_copies():
    X = iq_bank(True)[:777, :65]
    b = dsp.BankPowerDecimator(65, 1)
    assert b.out_rows(777) == 777
    assert same(call(b, X), np.ascontiguousarray(X))
    assert call(b, X[:0]).shape == (0, 65)


# ------------------------------------------------------- 5. rational resampler
# in, out -> mode, predec, interp, decim, ntaps (rational_resampler.h:121-167), rows out of 4200
RATIONAL = {(25000, 8000): ((0, 2, 16, 25, 1900), 1344), (32000, 8000): ((1, 4, 1, 1, 0), 1050), (10000, 8000): ((2, 1, 4, 5, 380), 3360),
            (8000, 8000): ((3, 1, 1, 1, 0), 4200), (8000, 12000): ((2, 1, 3, 2, 228), 6300)}


def rational_stages(ins, outs):
    """(interp, decim, taps) of every stage: the plan's decimating FIRs, then the polyphase resampler"""
    mode, predec, interp, decim, ntaps = RATIONAL[(ins, outs)][0]
    st = [(1, d, t) for d, t in dsp.decim_plan(predec)] if mode in (0, 1) else []
    if mode in (0, 2):
        bw = min(ins, outs) / 2.0
        taps = dsp.low_pass(bw, bw * 0.1, ins / predec * interp) * f32(interp)
        assert len(taps) == ntaps
        st.append((interp, decim, taps))
    return st


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ins,outs", sorted(RATIONAL))
@pytest.mark.parametrize("S", SHAPES)
def test_rational_resampler(S, ins, outs, cplx):
    plan, rows = RATIONAL[(ins, outs)]
    info = oracle.RationalResampler(ins, outs, cplx).info()
    assert tuple(info[n] for n in ("mode", "predec", "interp", "decim", "ntaps")) == plan
    stages = rational_stages(ins, outs)
    X = iq_bank(cplx)
    what = f"rational {ins} -> {outs} S={S} cplx={cplx}"
    cuts = chain_cuts(stages, cplx) if stages else cuts_for(0, (32, 32))
    Y = all_forms(lambda: dsp.BankRationalResampler(S, ins, outs, complex_data=cplx), X[:, :S], cuts, what)
    assert Y.shape == (rows, S)
    streams_differ(Y)
    npoly = 1 if plan[0] in (0, 2) else 0                       # the plan's decimating FIRs, then the resampler
    banks = [dsp.BankDecimatingFIR(S, t, d, complex_data=cplx) for i, d, t in stages[:len(stages) - npoly]]
    banks += [dsp.BankPolyphaseResampler(S, i, d, t, complex_data=cplx) for i, d, t in stages[len(stages) - npoly:]]
    Z = run_stages(banks, X[:, :S])
    assert same(Y, np.ascontiguousarray(Z)), f"{what}: differs from its stages run as separate banks"
    refs = oracle_columns(("rres", ins, outs, cplx), lambda: oracle.RationalResampler(ins, outs, cplx), X)
    worst = check_columns(Y, refs, lambda k: 5e-5, what)
    write_report("bank_rate_parity", {"test": "rational_resampler", "in": ins, "out": outs, "S": S, "frames": FRAMES, "complex": cplx,
                                      "rows": rows, "max_abs_err": worst * 5e-5, "bound": 5e-5})


def test_rational_known_answer_per_stream():
    """25000 -> 8000 at S = 65: stream k carries a tone of its own below 3 kHz; the strongest bin of its output is
    that tone at the new rate."""
    S, ins, outs, N = 65, 25000, 8000, 1024
    tone = lambda k: 200.0 + 40.0 * k
    assert tone(S - 1) < 3000
    n = np.arange(FRAMES)
    X = np.stack([np.exp(2j * np.pi * tone(k) * n / ins) for k in range(S)], axis=1).astype(np.complex64)
    Y = call(dsp.BankRationalResampler(S, ins, outs), X)
    assert len(Y) == 1344
    w = np.hanning(N)
    for k in range(S):
        peak = int(np.argmax(np.abs(np.fft.fft(Y[300:300 + N, k] * w))))   # (past the filters' transient)
        assert abs(peak - tone(k) / outs * N) <= 1.0, f"stream {k}: strongest bin {peak}, its tone is bin {tone(k) / outs * N:.1f}"


# -------------------------------------------------------------------- 6. reset
@pytest.mark.parametrize("name", ["decimating_fir", "polyphase", "power_decimator", "rational"])
def test_reset_reproduces_the_first_run(name):
    S = 65
    make = {"decimating_fir": lambda: dsp.BankDecimatingFIR(S, DFIR_TAPS["plan69"](), 7),
            "polyphase": lambda: dsp.BankPolyphaseResampler(S, 4, 5, poly_taps(4, 5)),
            "power_decimator": lambda: dsp.BankPowerDecimator(S, 8),
            "rational": lambda: dsp.BankRationalResampler(S, 25000, 8000)}[name]
    X = noise_bank(True)[:1001, :S]                              # (1001: no multiple of 7, 5, 8 or 25: phase and offset are carried)
    b = make()
    first = call(b, X)
    again = call(b, X)
    assert first.shape != again.shape or not same(again, first), "the state does not matter here: the check would show nothing"
    b.reset()
    assert same(call(b, X), first)


# -------------------------------------------- 7. channelizer -> bank on the device
def test_channelizer_feeds_rational_bank_by_device_pointer():
    import torch
    M, NF, ins, outs = 256, 1200, 25000, 8000
    h = dsp.windowed_sinc(16 * M, np.pi / M)                     # tests/test_channelizer.py
    rng = np.random.default_rng(5)
    x = iq(rng, NF * M)
    s = torch.cuda.Stream()
    d_x = torch.from_numpy(x.view(f32)).cuda()
    d_ch = torch.empty(2 * NF * M, dtype=torch.float32, device="cuda")
    bank = dsp.BankRationalResampler(M, ins, outs)
    rows = bank.out_rows(NF)
    assert rows == NF * 16 // 50
    d_y = torch.zeros(2 * rows * M, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ch = dsp.PolyphaseChannelizer(M, h)
    assert ch.process_dev(d_x.data_ptr(), NF * M, d_ch.data_ptr(), s.cuda_stream) == NF * M
    assert bank.process_dev(d_ch.data_ptr(), NF, d_y.data_ptr(), s.cuda_stream) == rows
    s.synchronize()
    assert np.all(bank.counts == rows)
    C = d_ch.cpu().numpy().view(np.complex64).reshape(NF, M)
    Y = d_y.cpu().numpy().view(np.complex64).reshape(rows, M)
    assert 0 < np.abs(C).max() <= 1.0                            # (the single-stream bar is for samples within the unit circle)
    assert same(Y, call(dsp.BankRationalResampler(M, ins, outs), C)), "fed by device pointer and fed a host copy differ"
    worst = 0.0
    for k in range(M):
        ref = dsp.RationalResampler(ins, outs).process(np.ascontiguousarray(C[:, k]))
        assert len(ref) == rows, f"channel {k}"
        worst = max(worst, float(np.abs(Y[:, k] - ref).max()))
        assert worst <= 5e-5, f"channel {k}: max abs err {worst:.3e}"
    write_report("bank_rate_parity", {"test": "channelizer_to_rational", "channels": M, "frames": NF, "rows": rows, "max_abs_err": worst,
                                      "bound": 5e-5})


# ---------------------------------------------------------- 8. counts and sizes
def test_out_rows_follow_the_phase():
    b = dsp.BankDecimatingFIR(3, np.ones(4, f32), 7, complex_data=False)
    assert b.streams == 3 and b.out_rows(0) == 0 and b.out_rows(1) == 1 and b.out_rows(7) == 1 and b.out_rows(8) == 2
    assert call(b, np.ones((3, 3), f32)).shape == (1, 3)         # row 0; the next output is 4 rows on
    assert b.out_rows(4) == 0 and b.out_rows(5) == 1
    assert call(b, np.ones((4, 3), f32)).shape == (0, 3) and list(b.counts) == [0, 0, 0]
    assert b.out_rows(1) == 1
    up = dsp.BankPolyphaseResampler(3, 3, 2, np.ones(6, f32), complex_data=False)
    assert up.out_rows(100) == 150 and call(up, np.ones((100, 3), f32)).shape == (150, 3)
    with pytest.raises(ValueError):
        up.process(np.ones((5, 4), f32))
    with pytest.raises(sdrpp_amd.SdrGpuError):
        up.out_rows(2 ** 29)                                    # 2^29 rows in fit (3 streams), the 1.5 x 2^29 rows out do not
    with pytest.raises(sdrpp_amd.SdrGpuError):
        up.process_dev(1, 2 ** 29, 1)
