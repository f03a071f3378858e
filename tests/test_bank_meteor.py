"""The carrier-loop banks and the Meteor receiver bank on the device (libsdrgpu, HIP): S streams per launch in the
channelizer's layout x[m, k], one lane per stream.

The reference of every bank column is a fresh SINGLE-STREAM handle of the block with the same parameters, fed that
column in one call (those blocks are held to the reference by tests/test_meteor.py and tests/test_meteor_ref.py): no bar
here comes from a bank's own numbers.

* BankPLL, BankCarrierPLL, BankMeteorCostas (both errors), BankMeteor (outputs and counts[k], the four (broken, oqpsk)
  combinations) -- every column bit-identical to its single-stream handle; elements of a BankMeteor row past a stream's
  count keep the sentinel `out` held; banks in cuts bit-identical to whole runs.
* BankMeteor -- bit-identical to bank FIR -> bank FastAGC -> bank MeteorCostas -> the stagger in numpy -> bank MM.
* reset keeps the per-stream stagger carry and MM's history, as the single-stream block.
* A channelizer's device output feeds a BankMeteor by pointer.
* Known answer at S = 65: where the single-stream dsp.Meteor recovers a stream without error, the bank does too.
* Shapes, cuts and the sentinel are tests/test_banks.py's: S in {1, 63, 64, 65, 130}, 4200 frames. Stream k differs from
  every other in seed, amplitude, carrier offset and phase, and columns are compared one by one: swapped streams fail."""
import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import dsp
from _restated import same, errors_at_best_lag, quadrant
from test_banks import (FRAMES, SHAPES, SMAX, SENTINEL, cached, single_columns, run_whole, whole_and_cut, check_columns,
                        streams_differ)
import _meteor as M

pytestmark = pytest.mark.gpu
f32 = np.float32
COMBOS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"


def lrpt_bank(kind, unit=False, S=SMAX):
    return cached(("lrpt", kind, unit, S), lambda: M.bank_streams(S, kind, n=FRAMES, unit=unit))


def carriers():
    return cached(("carriers",), lambda: M.bank_carriers(SMAX, n=FRAMES))


# --------------------------------------------- 1. bit-identical to single streams
@pytest.mark.parametrize("derotate", [False, True])
@pytest.mark.parametrize("S", SHAPES)
def test_pll_columns(S, derotate):
    X = carriers()
    single, bank = (dsp.CarrierPLL, dsp.BankCarrierPLL) if derotate else (dsp.PLL, dsp.BankPLL)
    refs = single_columns(("pll", derotate), lambda: single(M.LOOP_BW), X)
    what = f"{'carrier_' if derotate else ''}pll S={S}"
    ys, c = whole_and_cut(lambda: bank(S, M.LOOP_BW), X[:, :S], what)
    assert np.all(c == FRAMES)
    streams_differ(refs[:S])
    check_columns(ys, refs[:S], what)


@pytest.mark.parametrize("broken", [False, True])
@pytest.mark.parametrize("S", SHAPES)
def test_meteor_costas_columns(S, broken):
    X = lrpt_bank("broken" if broken else "qpsk", unit=True)[0]
    refs = single_columns(("mcostas", broken), lambda: dsp.MeteorCostas(M.COSTAS_BW, broken), X)
    ys, _ = whole_and_cut(lambda: dsp.BankMeteorCostas(S, M.COSTAS_BW, broken), X[:, :S], f"meteor_costas broken={broken} S={S}")
    streams_differ(refs[:S])
    check_columns(ys, refs[:S], f"meteor_costas broken={broken} S={S}")
    if not broken:                                              # ... and with it Costas<4>'s bank
        zs, _ = run_whole(dsp.BankCostas(S, 4, M.COSTAS_BW), X[:, :S])
        check_columns(ys, zs, f"meteor_costas S={S} against BankCostas<4>")


def signal_of(broken, oqpsk):
    return "broken" if broken else ("oqpsk" if oqpsk else "qpsk")


@pytest.mark.parametrize("broken,oqpsk", COMBOS)
@pytest.mark.parametrize("S", SHAPES)
def test_meteor_columns_and_counts(S, broken, oqpsk):
    X = lrpt_bank(signal_of(broken, oqpsk))[0]
    args = M.meteor_args(broken, oqpsk)
    refs = single_columns(("meteor", broken, oqpsk), lambda: dsp.Meteor(*args), X)
    what = f"meteor broken={broken} oqpsk={oqpsk} S={S}"
    ys, c = whole_and_cut(lambda: dsp.BankMeteor(S, *args), X[:, :S], what)    # (run_whole checks the sentinel past the counts)
    assert list(c) == [len(r) for r in refs[:S]], f"{what}: counts"
    streams_differ(refs[:S])
    check_columns(ys, refs[:S], what)


# ----------------------------------------------- 2. the composite is its stages
def stagger(ys, last_i):
    """meteor_demod.h:155-161 per stream on the host: the Q arm one sample late, last_i [S] carried."""
    out = []
    for k, y in enumerate(ys):
        im = np.concatenate([[last_i[k]], y.imag]).astype(f32)
        if len(y):
            last_i[k] = im[-1]
        out.append((y.real + 1j * im[:-1]).astype(np.complex64))
    return out


def as_rows(ys, S):
    X = np.zeros((max(len(y) for y in ys), S), np.complex64)
    for k, y in enumerate(ys):
        X[:len(y), k] = y
    return X


@pytest.mark.parametrize("broken,oqpsk", COMBOS)
@pytest.mark.parametrize("S", SHAPES)
def test_bank_meteor_is_its_stages(S, broken, oqpsk):
    X = lrpt_bank(signal_of(broken, oqpsk))[0][:, :S]
    a = M.meteor_args(broken, oqpsk)
    ys, c = run_whole(dsp.BankMeteor(S, *a), X)
    stages = [dsp.BankFIR(S, dsp.root_raised_cosine(a[2], a[3], a[1] / a[0])), dsp.BankFastAGC(S, 1.0, 10e6, a[4], complex_data=True),
              dsp.BankMeteorCostas(S, a[5], broken)]
    Z = X
    for b in stages:
        zs, _ = run_whole(b, Z)
        Z = as_rows(zs, S)
    if oqpsk:
        Z = as_rows(stagger(zs, np.zeros(S, f32)), S)
    zs, d = run_whole(dsp.BankMM(S, a[1] / a[0], a[8], a[9], a[10], complex_data=True), Z)
    assert list(c) == list(d) and all(abs(n - FRAMES * M.DOWN // M.UP) <= 3 for n in c)
    check_columns(ys, zs, f"meteor stages broken={broken} oqpsk={oqpsk} S={S}")


# -------------------------------------------------------------------- 3. reset
def test_reset_keeps_the_stagger_carry_and_mm_history():
    S = 65
    X = lrpt_bank("oqpsk")[0][:, :S]
    args = M.meteor_args(False, True)
    b, singles = dsp.BankMeteor(S, *args), [dsp.Meteor(*args) for _ in range(S)]
    for lo, hi in ((0, 2001), (2001, FRAMES)):
        ys, c = run_whole(b, X[lo:hi])
        refs = [m.process(np.ascontiguousarray(X[lo:hi, k])) for k, m in enumerate(singles)]
        check_columns(ys, refs, f"meteor reset rows {lo}..{hi}")
        b.reset()
        for m in singles:
            m.reset()
    fresh = dsp.Meteor(*args).process(np.ascontiguousarray(X[2001:, 0]))
    assert not same(refs[0][:2], fresh[:2]), "the carry and the history do not matter here: the check would show nothing"


@pytest.mark.parametrize("name", ["pll", "carrier_pll", "meteor_costas"])
def test_loop_bank_reset_reproduces_the_first_run(name):
    S = 65
    make, X = {"pll": (lambda: dsp.BankPLL(S, M.LOOP_BW), carriers()),
               "carrier_pll": (lambda: dsp.BankCarrierPLL(S, M.LOOP_BW), carriers()),
               "meteor_costas": (lambda: dsp.BankMeteorCostas(S, M.COSTAS_BW, True), lrpt_bank("broken", unit=True)[0])}[name]
    X = X[:1000, :S]
    b = make()
    first = b.process(X).copy()
    b.reset()
    assert same(b.process(X), first)
    assert not same(b.process(X), first), "the state does not matter here: the check would show nothing"


# ------------------------------------------------------------ 4. known answers
def test_known_answer_per_stream():
    S, lo, hi = 65, 600, 1800
    X, qs = lrpt_bank("qpsk", S=65)
    args = M.meteor_args(False, False)
    score = lambda y, k: errors_at_best_lag(np.diff(quadrant(y)) % 4, np.diff(qs[k]) % 4, range(40), lo, hi)[0]
    good = [k for k in range(S) if score(dsp.Meteor(*args).process(np.ascontiguousarray(X[:, k])), k) == 0]
    assert len(good) >= S - 2, f"condition: dsp.Meteor recovers only {len(good)} of {S} streams"
    ys, c = run_whole(dsp.BankMeteor(S, *args), X)
    errs = [score(ys[k], k) for k in good]
    print(f"meteor bank: {len(good)} streams, errors {errs}, counts {c.min()}..{c.max()}")
    assert errs == [0] * len(good)


# ------------------------------------------- 5. channelizer -> bank on the device
def test_channelizer_feeds_a_meteor_bank_by_device_pointer():
    import torch
    Mch, NF = 256, 1200
    h = dsp.windowed_sinc(16 * Mch, np.pi / Mch)                 # tests/test_channelizer.py
    rng = np.random.default_rng(6)
    x = (rng.uniform(-1, 1, NF * Mch) + 1j * rng.uniform(-1, 1, NF * Mch)).astype(np.complex64)
    s = torch.cuda.Stream()
    d_x = torch.from_numpy(x.view(f32)).cuda()
    d_ch = torch.empty(2 * NF * Mch, dtype=torch.float32, device="cuda")
    d_y = torch.full((2 * NF * Mch,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ch = dsp.PolyphaseChannelizer(Mch, h)
    assert ch.process_dev(d_x.data_ptr(), NF * Mch, d_ch.data_ptr(), s.cuda_stream) == NF * Mch
    args = M.meteor_args(True, True)
    bank = dsp.BankMeteor(Mch, *args)
    rows = bank.process_dev(d_ch.data_ptr(), NF, d_y.data_ptr(), s.cuda_stream)
    s.synchronize()
    C = d_ch.cpu().numpy().view(np.complex64).reshape(NF, Mch)
    Y = d_y.cpu().numpy().view(np.complex64).reshape(NF, Mch)
    c = bank.counts
    assert np.abs(C).max() > 0 and rows == c.max() and abs(int(c.min()) - NF * M.DOWN // M.UP) <= 3
    sentinel = np.array([SENTINEL, SENTINEL], f32).view(np.complex64)[0]
    for k in range(Mch):
        want = dsp.Meteor(*args).process(np.ascontiguousarray(C[:, k]))
        assert c[k] == len(want) and same(np.ascontiguousarray(Y[:c[k], k]), want), f"channel {k}"
        assert np.all(Y[c[k]:, k] == sentinel)
