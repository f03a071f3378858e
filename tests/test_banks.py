"""Stream banks on the device (libsdrgpu, HIP): S streams per launch in the channelizer's layout
x[m, k], one lane per stream.

The reference of every bank column is a fresh SINGLE-STREAM handle of the existing block with the same
parameters, fed that column in one call. Those blocks are held to the reference by tests/test_symsync.py
and tests/test_gpu_parity.py; no bar here comes from a bank's own numbers.

Bars:
* Quadrature, FastAGC, Costas<2|4|8>, MM (outputs and counts[k]) -- every column bit-identical to its
  single-stream handle. Elements of an MM row past a stream's count keep the sentinel `out` held.
* FIR -- every column within fir_atol(taps, x) of the fp64-accumulated correlation; the impulse response
  is the taps in correlation order, exactly; cuts bit-identical to the whole.
* BankPSK<4>, BankGFSK -- bit-identical to their bank stages run one after another.
* Known answers at S = 65: where the single-stream dsp.PSK / dsp.GFSK recovers every stream's symbols
  without error, so must the bank.
* Channelizer -> bank by device pointer.
* Shapes: S in {1, 63, 64, 65, 130} (one stream, a partial wave, a full wave, a wave and a lane, three
  waves with a ragged last), 4200 frames. Every streaming test runs a bank whole and a fresh one over
  CUTS (one row, the T - 1 = 7 history edge, an empty call, the kernels' 32-row tile edge, 1024) and
  requires the same bits.
* Stream k's data differs from every other stream's (seed, scale; for the PSK signals also amplitude,
  carrier offset and phase) and columns are compared one by one: swapped streams fail.
The parity summary goes to bank_parity.jsonl through write_report.
"""
import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import dsp
from _util import fir_atol, write_report
from _restated import same, shaped_psk, gfsk_signal, errors_at_best_lag, quadrant, ref_slicer, GFSK_ARGS

pytestmark = pytest.mark.gpu

f32 = np.float32
FRAMES = 4200
SHAPES = [1, 63, 64, 65, 130]
SMAX = max(SHAPES)
TILE = 32                                                       # bank_kernels.h BANK_F
CUTS = [1, 6, 7, 8, 0, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1]
CUTS = CUTS + [FRAMES - sum(CUTS)]
SENTINEL = -12345.0
PSK_ARGS = (4, 1.0, 4.0, 31, 0.6, 0.01, 0.005, 2.5e-5, 0.01, 0.01)


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
    """(FRAMES, SMAX): stream k is uniform noise from default_rng(100 + k) scaled by 0.25 + 0.25 (k mod 8)."""
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


def psk_params(k):
    """seed, amplitude in [0.2, 2], carrier offset in +-3e-4 cycles/sample, phase of stream k"""
    return dict(seed=200 + k, amp=0.2 + 1.8 * ((k * 37) % SMAX) / (SMAX - 1), cfo=3e-4 * (((k * 53) % 131) / 65.0 - 1.0),
                phase=0.1 * k)


def psk_bank(order, nsym=FRAMES // 4, S=SMAX):
    def make():
        cols = [shaped_psk(order=order, nsym=nsym, **psk_params(k)) for k in range(S)]
        return np.ascontiguousarray(np.stack([c[0] for c in cols], axis=1)), [c[1] for c in cols]
    return cached(("psk", order, nsym, S), make)


def gfsk_bank(nsym, S):
    def make():
        cols = [gfsk_signal(seed=300 + k, nsym=nsym) for k in range(S)]
        return np.ascontiguousarray(np.stack([c[0] for c in cols], axis=1)), [c[1] for c in cols]
    return cached(("gfsk", nsym, S), make)


def single_columns(key, make_single, X):
    """The reference, once per configuration: column k of X through a fresh single-stream handle."""
    return cached(("ref",) + key, lambda: [make_single().process(np.ascontiguousarray(X[:, k])) for k in range(X.shape[1])])


# ------------------------------------------------------------ running banks
def run_whole(bank, X):
    """One call; returns the per-stream outputs (out[:counts[k], k]) and checks the sentinel past them."""
    out = np.full((max(bank.out_rows(len(X)), 1), bank.streams), SENTINEL, bank.out_dtype)
    y = bank.process(X, out=out)
    c = bank.counts
    assert c.dtype == np.int32 and c.shape == (bank.streams,)
    assert len(y) == (c.max() if len(X) else 0)
    for k in range(bank.streams):
        assert np.all(out[c[k]:, k] == out.dtype.type(SENTINEL)), f"stream {k}: rows past its count were written"
    return [np.ascontiguousarray(y[:c[k], k]) for k in range(bank.streams)], c


def run_cuts(bank, X):
    parts, i = [[] for _ in range(bank.streams)], 0
    for n in CUTS:
        ys, _ = run_whole(bank, X[i:i + n])
        for k, y in enumerate(ys):
            parts[k].append(y)
        i += n
    assert i == len(X) == FRAMES
    return [np.concatenate(p) for p in parts]


def whole_and_cut(make, X, what):
    ys, c = run_whole(make(), X)
    zs = run_cuts(make(), X)
    for k, (y, z) in enumerate(zip(ys, zs)):
        assert same(y, z), f"{what}: stream {k} in calls differs from one call"
    return ys, c


def check_columns(ys, refs, what):
    for k, y in enumerate(ys):
        assert len(y) == len(refs[k]), f"{what}: stream {k} made {len(y)} outputs, its single-stream handle {len(refs[k])}"
        assert same(y, refs[k]), f"{what}: stream {k} differs from its single-stream handle"


def streams_differ(refs):
    assert len(refs) < 2 or not any(len(refs[0]) == len(r) and same(refs[0], r) for r in refs[1:]), "streams with equal outputs show nothing"


# --------------------------------------------- 1. bit-identical to single streams
@pytest.mark.parametrize("S", SHAPES)
def test_quadrature_columns(S):
    X = noise_bank(True)
    refs = single_columns(("quad",), lambda: dsp.Quadrature(0.4), X)
    ys, c = whole_and_cut(lambda: dsp.BankQuadrature(S, 0.4), X[:, :S], f"quadrature S={S}")
    assert np.all(c == FRAMES) and ys[0].dtype == f32
    streams_differ(refs[:S])
    check_columns(ys, refs[:S], f"quadrature S={S}")


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("S", SHAPES)
def test_fast_agc_columns(S, cplx):
    X = noise_bank(cplx)
    args = (1.0, 3.0, 0.1, 2.0)                                 # setPoint, maxGain, rate, initGain: the gain meets maxGain
    refs = single_columns(("agc", cplx), lambda: dsp.FastAGC(*args, complex_data=cplx), X)
    ys, _ = whole_and_cut(lambda: dsp.BankFastAGC(S, *args, complex_data=cplx), X[:, :S], f"fast_agc S={S} cplx={cplx}")
    streams_differ(refs[:S])
    check_columns(ys, refs[:S], f"fast_agc S={S} cplx={cplx}")


@pytest.mark.parametrize("order", [2, 4, 8])
@pytest.mark.parametrize("S", SHAPES)
def test_costas_columns(S, order):
    X, _ = psk_bank(order)
    refs = single_columns(("costas", order), lambda: dsp.Costas(order, 0.005), X)
    ys, _ = whole_and_cut(lambda: dsp.BankCostas(S, order, 0.005), X[:, :S], f"costas<{order}> S={S}")
    streams_differ(refs[:S])
    check_columns(ys, refs[:S], f"costas<{order}> S={S}")


# omega, omegaGain, muGain, bank. With the gains of tests/test_symsync.py the 998 outputs of omega = 5000 / 1187.5 come
# out equal for every noise stream (the restatement, on the CPU): livelier gains there, under which the counts
# of the first 8 streams spread over 991..1005.
MM_CASES = [(om, og, mg, P, T) for om, og, mg in ((4.0, 2.5e-5, 0.01), (5000.0 / 1187.5, 1e-3, 0.05)) for P, T in ((128, 8), (4, 3))]


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("om,og,mg,P,T", MM_CASES)
@pytest.mark.parametrize("S", SHAPES)
def test_mm_columns_and_counts(S, om, og, mg, P, T, cplx):
    X = noise_bank(cplx)
    args = (om, og, mg, 0.01, P, T)
    refs = single_columns(("mm", om, P, T, cplx), lambda: dsp.MM(*args, complex_data=cplx), X)
    lens = [len(r) for r in refs]
    assert len(set(lens[:8])) > 1, f"precondition: the single-stream counts of the first streams are all equal ({lens[0]})"
    what = f"mm S={S} omega={om} bank=({P}, {T}) cplx={cplx}"
    ys, c = whole_and_cut(lambda: dsp.BankMM(S, *args, complex_data=cplx), X[:, :S], what)
    assert list(c) == lens[:S], f"{what}: counts"
    check_columns(ys, refs[:S], what)


# ------------------------------------------------------------------- 2. FIR
FIR_TAPS = {"rrc31": lambda: dsp.root_raised_cosine(31, 0.6, 4.0),
            "ramp8": lambda: (np.arange(1, 9) / 8.0).astype(f32) * np.array([1, -1, 1, 1, -1, 1, -1, -1], f32)}


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("name", sorted(FIR_TAPS))
@pytest.mark.parametrize("S", SHAPES)
def test_fir_columns(S, name, cplx):
    taps = FIR_TAPS[name]()
    X = noise_bank(cplx)[:, :S]
    what = f"fir {name} S={S} cplx={cplx}"
    ys, _ = whole_and_cut(lambda: dsp.BankFIR(S, taps, complex_data=cplx), X, what)
    worst = 0.0
    for k, y in enumerate(ys):
        x = X[:, k].astype(np.complex128 if cplx else np.float64)
        ref = np.convolve(x, taps.astype(np.float64)[::-1])[:FRAMES]     # [T - 1 zeros || x] correlated with the taps
        err, tol = np.abs(y.astype(ref.dtype) - ref).max(), fir_atol(taps, X[:, k])
        worst = max(worst, err / tol)
        assert err <= tol, f"{what}: stream {k} max abs err {err:.3e} > {tol:.3e}"
    write_report("bank_parity", {"test": "fir", "taps": name, "S": S, "frames": FRAMES, "complex": cplx, "max_err_over_bound": worst})


@pytest.mark.parametrize("cplx", [False, True])
def test_fir_impulse_response(cplx):
    S, taps = 65, FIR_TAPS["rrc31"]()
    T = len(taps)
    X = np.zeros((64, S), np.complex64 if cplx else f32)
    for k in range(S):
        X[k % 7, k] = f32(2.0 ** (k % 5)) * (1j if cplx and k % 2 else 1)      # an exact scale, its own row per stream
    y = dsp.BankFIR(S, taps, complex_data=cplx).process(X)
    for k in range(S):
        want = np.zeros(64, X.dtype)
        want[k % 7:k % 7 + T] = X[k % 7, k] * taps[::-1]          # out[m] = sum_j buf[m + j] taps[j]: tap T - 1 first
        assert same(y[:, k] + 0, want + 0), f"stream {k}"         # (+ 0: -0.0 and 0.0 are the same answer)


# ----------------------------------------------- 3. composites are their stages
def run_stages(stages, X):
    c = None
    for b in stages:
        ys, c = run_whole(b, X)
        X = np.zeros((int(c.max()), b.streams), b.out_dtype)
        for k, y in enumerate(ys):
            X[:len(y), k] = y
    return ys, c


def psk_stages(S):
    return [dsp.BankFIR(S, dsp.root_raised_cosine(31, 0.6, 4.0)), dsp.BankFastAGC(S, 1.0, 10e6, 0.01, complex_data=True),
            dsp.BankCostas(S, 4, 0.005), dsp.BankMM(S, 4.0, 2.5e-5, 0.01, 0.01, complex_data=True)]


def gfsk_stages(S, dev_rad=2 * np.pi * 3000.0 / 48000.0):
    return [dsp.BankQuadrature(S, dev_rad), dsp.BankFIR(S, dsp.root_raised_cosine(31, 0.6, 4.0), complex_data=False),
            dsp.BankMM(S, 4.0, 2.5e-5, 0.01, 0.01)]


@pytest.mark.parametrize("S", SHAPES)
def test_bank_psk_is_its_stages(S):
    X = psk_bank(4)[0][:, :S]
    ys, c = whole_and_cut(lambda: dsp.BankPSK(S, *PSK_ARGS), X, f"psk S={S}")
    zs, d = run_stages(psk_stages(S), X)
    assert list(c) == list(d) and all(abs(n - FRAMES // 4) <= 3 for n in c)
    check_columns(ys, zs, f"psk S={S}")


@pytest.mark.parametrize("S", SHAPES)
def test_bank_gfsk_is_its_stages(S):
    X = gfsk_bank(FRAMES // 4, SMAX)[0][:, :S]
    ys, c = whole_and_cut(lambda: dsp.BankGFSK(S, *GFSK_ARGS), X, f"gfsk S={S}")
    zs, d = run_stages(gfsk_stages(S), X)
    assert ys[0].dtype == f32 and list(c) == list(d)
    check_columns(ys, zs, f"gfsk S={S}")


# ------------------------------------------------------------ 4. known answers
KA_S, KA_NSYM, KA_LO, KA_HI = 65, 2000, 600, 1800


def test_qpsk_known_answer_per_stream():
    X, qs = psk_bank(4, KA_NSYM, KA_S)
    dqs = [np.diff(q) % 4 for q in qs]
    score = lambda y, k: errors_at_best_lag(np.diff(quadrant(y)) % 4, dqs[k], range(40), KA_LO, KA_HI)[0]
    for k in range(KA_S):                                       # the condition: the single-stream handle recovers every stream
        y = dsp.PSK(*PSK_ARGS).process(np.ascontiguousarray(X[:, k]))
        assert score(y, k) == 0, f"condition: dsp.PSK does not recover stream {k} ({psk_params(k)})"
    ys, c = run_whole(dsp.BankPSK(KA_S, *PSK_ARGS), X)
    errs = [score(y, k) for k, y in enumerate(ys)]
    print(f"qpsk bank: errors {errs}, counts {c.min()}..{c.max()}")
    assert errs == [0] * KA_S


def test_gfsk_known_answer_per_stream():
    X, bs = gfsk_bank(KA_NSYM, KA_S)
    score = lambda y, k: errors_at_best_lag(ref_slicer(y), bs[k].astype(np.uint8), range(40), KA_LO, KA_HI)[0]
    for k in range(KA_S):
        y = dsp.GFSK(*GFSK_ARGS).process(np.ascontiguousarray(X[:, k]))
        assert score(y, k) == 0, f"condition: dsp.GFSK does not recover stream {k}"
    ys, c = run_whole(dsp.BankGFSK(KA_S, *GFSK_ARGS), X)
    errs = [score(y, k) for k, y in enumerate(ys)]
    print(f"gfsk bank: errors {errs}, counts {c.min()}..{c.max()}")
    assert errs == [0] * KA_S


# ------------------------------------------- 5. channelizer -> bank on the device
def test_channelizer_feeds_banks_by_device_pointer():
    import torch
    M, NF = 256, 1200
    h = dsp.windowed_sinc(16 * M, np.pi / M)                     # tests/test_channelizer.py
    rng = np.random.default_rng(5)
    x = (rng.uniform(-1, 1, NF * M) + 1j * rng.uniform(-1, 1, NF * M)).astype(np.complex64)
    s = torch.cuda.Stream()
    d_x = torch.from_numpy(x.view(f32)).cuda()
    d_ch = torch.empty(2 * NF * M, dtype=torch.float32, device="cuda")
    d_q = torch.empty(NF * M, dtype=torch.float32, device="cuda")
    d_g = torch.full((NF * M,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ch = dsp.PolyphaseChannelizer(M, h)
    assert ch.process_dev(d_x.data_ptr(), NF * M, d_ch.data_ptr(), s.cuda_stream) == NF * M
    quad, gfsk = dsp.BankQuadrature(M, 0.4), dsp.BankGFSK(M, *GFSK_ARGS)
    assert quad.process_dev(d_ch.data_ptr(), NF, d_q.data_ptr(), s.cuda_stream) == NF
    rows = gfsk.process_dev(d_ch.data_ptr(), NF, d_g.data_ptr(), s.cuda_stream)
    s.synchronize()
    C = d_ch.cpu().numpy().view(np.complex64).reshape(NF, M)
    Q = d_q.cpu().numpy().reshape(NF, M)
    G = d_g.cpu().numpy().reshape(NF, M)
    assert np.abs(C).max() > 0
    for k in range(M):
        assert same(np.ascontiguousarray(Q[:, k]), dsp.Quadrature(0.4).process(np.ascontiguousarray(C[:, k]))), f"channel {k}"
    c = gfsk.counts
    assert rows == c.max() and abs(int(c.min()) - NF // 4) <= 3
    zs, d = run_stages(gfsk_stages(M), C)
    assert list(c) == list(d)
    for k in range(M):
        assert same(np.ascontiguousarray(G[:c[k], k]), zs[k]), f"channel {k}"
        assert np.all(G[c[k]:, k] == f32(SENTINEL))


# -------------------------------------------------------------------- 6. reset
@pytest.mark.parametrize("name", ["quadrature", "fir", "fast_agc", "costas", "fir_real"])
def test_reset_reproduces_the_first_run(name):
    S = 65
    make, X = {
        "quadrature": (lambda: dsp.BankQuadrature(S, 0.4), noise_bank(True)),
        "fir": (lambda: dsp.BankFIR(S, FIR_TAPS["rrc31"]()), noise_bank(True)),
        "fast_agc": (lambda: dsp.BankFastAGC(S, 1.0, 3.0, 0.1, 2.0), noise_bank(False)),
        "costas": (lambda: dsp.BankCostas(S, 4, 0.005), psk_bank(4)[0]),
        "fir_real": (lambda: dsp.BankFIR(S, FIR_TAPS["ramp8"](), complex_data=False), noise_bank(False)),
    }[name]
    X = X[:1000, :S]
    b = make()
    first = b.process(X).copy()
    b.reset()
    assert same(b.process(X), first)
    assert not same(b.process(X), first), "the state does not matter here: the check would show nothing"


@pytest.mark.parametrize("cplx", [False, True])
def test_mm_reset_keeps_history(cplx):
    """mm.h:87-98: reset restores the loop state, the T - 1 history rows stay -- as the single-stream block."""
    S = 65
    X = noise_bank(cplx)[:, :S]
    args = (4.0, 2.5e-5, 0.01, 0.01)
    b = dsp.BankMM(S, *args, complex_data=cplx)
    singles = [dsp.MM(*args, complex_data=cplx) for _ in range(S)]
    for lo, hi in ((0, 2001), (2001, FRAMES)):
        ys, c = run_whole(b, X[lo:hi])
        refs = [m.process(np.ascontiguousarray(X[lo:hi, k])) for k, m in enumerate(singles)]
        check_columns(ys, refs, f"mm reset cplx={cplx} rows {lo}..{hi}")
        b.reset()
        for m in singles:
            m.reset()
    fresh = dsp.MM(*args, complex_data=cplx).process(np.ascontiguousarray(X[2001:, 0]))
    assert not same(refs[0][:2], fresh[:2]), "the history does not matter here: the check would show nothing"


def test_counts_and_shapes_of_a_plain_bank():
    b = dsp.BankFastAGC(3, 1.0, 3.0, 0.1)
    assert b.streams == 3 and b.out_rows(17) == 17
    y = b.process(np.ones((5, 3), f32))
    assert y.shape == (5, 3) and list(b.counts) == [5, 5, 5]
    assert b.process(np.ones((0, 3), f32)).shape == (0, 3) and list(b.counts) == [0, 0, 0]
    with pytest.raises(ValueError):
        b.process(np.ones((5, 4), f32))
    with pytest.raises(sdrpp_amd.SdrGpuError):
        b.out_rows(2 ** 30)                                     # 3 * 2^30 rows * streams: past the kernels' int index
    with pytest.raises(sdrpp_amd.SdrGpuError):
        b.process_dev(1, 2 ** 30, 1)
