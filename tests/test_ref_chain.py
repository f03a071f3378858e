"""The channel chain pinned to the REFERENCE's own headers, setters and reset included:
tests/golden/ref_chain_*.npz hold what oracle/_ref/ref_blocks -- channel/frequency_xlator.h, rx_vfo.h,
filter/fir.h, decimating_fir.h, multirate/*.h, demod/quadrature.h and fm.h compiled over
oracle/ref_standins.cpp -- computes for FrequencyXlator, FIR / DecimatingFIR, PowerDecimator,
PolyphaseResampler, RationalResampler, RxVFO, Quadrature, FM and the literal chains xlator ->
DecimatingFIR [-> Quadrature] (tools/gen_ref_fixtures.py chain_cases). Every case is an op list: sample
counts (process() calls) and, mid-stream, `w<rad>` xlator setOffset, `f<hz>` RxVFO::setOffset, `d<n>`
setDecimation, `t<k>` setTaps to the k-th tap set, `v<rad>` setDeviation and `r` reset. It is fed twice:
every segment whole, and every segment in calls of 1, 0, a count below ntaps - 1, 7, 0, 129, 1025 and the
rest in two. Three builds of the reference are recorded: VOLK's dot products summed in ascending order,
in the order of a 4-lane SIMD kernel (_sum4), and ascending with the rotator's phase carried in fp64
(_rot64).

Bars, for the C oracle (precise mode, on the CPU) and for the dsp.* blocks (on the device):
* Output counts: exact, per call, in both feeds.
* Values: S = the largest gap between the reference's own builds on the fixture (ascending against
  _sum4; against _rot64 as well for xlator, ddc, ddcfm and rxvfo), over both feeds. Every output of
  both feeds within 16 max(S, 4 eps32 max|y|) of the ascending build: the bar and margin of the chains
  in test_ref_blocks.py (a summation order and a libm are one more rounding of the class S measures).
  S comes from the reference builds alone.
* Quadrature (quad): 8 spacing(pi) / dev, the bar test_ref_pinned.py holds the device's atan2f to (the
  input is exact, so nothing else enters). After a FIR (ddcfm): (2 bar_fir / min|z| + 8 spacing(pi)) /
  dev, z the reference's FIR-stage output, bar_fir the value bar on z, dev the deviation in force at
  that output; z itself is compared too, through the same chain without the demodulator, within bar_fir. FM is the quadrature of an exact input followed by a real FIR h (the audio filter), a
  linear map of gain at most sum|h|: sum|h| 8 spacing(pi) / dev for the quadrature, plus the value bar
  for the filter's own sums.
* Conditions on the fixtures, asserted here on the CPU (test_fixture_meets_the_conditions): the three
  builds give equal counts; for the random-tap cases every |h_k| rms(x) >= 64 bar, so no tap could be
  dropped or shifted inside the bar; every retune moves the output by |dw| rms(x) >= 1000 bar;
  min|z| >= 0.25 for ddcfm; and every output of every call is compared (the compared length is the
  sum of the counts).
Against the pinned oracle, at the sizes where the host takes another path: RxVFO in the C5 shape over
calls of 1,200,000, 307,200 and 999 samples with set_offset and reset between them, and the FIR walk at
200,000 samples per segment, within test_gpu_parity.py's bars for the same blocks (5e-5, fir_atol).
Recorded: profiles/r19/ref_pin_chain.json.
"""
import glob
import os

import numpy as np
import pytest

import oracle
from sdrpp_amd import dsp
from _util import EPS32, GOLDEN, assert_close_c, assert_live_probe_reproduces, fir_atol, have_reference, iq, write_report

gpu = pytest.mark.gpu
FEEDS = ("whole", "cut")
ATAN_BAR = 8 * float(np.spacing(np.float32(np.pi)))
CASES = ["ddc", "ddcfm", "fir_cc", "fir_real", "fir_walk", "fm_bp", "fm_lp", "pdec_256_c", "pdec_64_c", "pdec_64_f",
         "poly_1_7_c", "poly_1_7_f", "poly_3_2_c", "poly_3_2_f", "poly_5_4_c", "poly_5_4_f", "quad", "rres_both",
         "rres_decim", "rres_none", "rres_resamp", "rxvfo_c5", "rxvfo_d64", "rxvfo_poly", "xlator"]
RANDOM_TAPS = [c for c in CASES if c.startswith(("fir_", "poly_")) or c == "ddc"]
ROTATOR = ("xlator", "ddc", "ddcfm", "rxvfo")


def load(name):
    """The case's arrays (the cut feed's outputs lie in a second file where one would be too large)."""
    g = {}
    for path in (f"ref_chain_{name}.npz", f"ref_chain_{name}_cut.npz"):
        if os.path.exists(os.path.join(GOLDEN, path)):
            with np.load(os.path.join(GOLDEN, path)) as f:
                g.update({k: f[k] for k in f.files})
    g["x"] = from_i16(g["xi16"])
    g["taps"] = [g[f"taps{k}"] for k in range(sum(k.startswith("taps") for k in g))]
    g["mode"] = str(g["mode"])
    return g


def from_i16(k):
    x = (np.asarray(k, np.float32) / np.float32(32768.0)).astype(np.float32)
    return np.ascontiguousarray(x).view(np.complex64)[:, 0] if x.ndim == 2 else x


def test_the_case_list_is_the_fixtures():
    on_disk = {os.path.basename(p)[len("ref_chain_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "ref_chain_*.npz"))}
    assert {c for c in on_disk if not (c.endswith("_cut") and c[:-4] in on_disk)} == set(CASES)


def gap(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    if not a.size:
        return 0.0
    if np.iscomplexobj(a):
        return float(max(np.abs(a.real.astype(np.float64) - b.real).max(), np.abs(a.imag.astype(np.float64) - b.imag).max()))
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


def own_gap(g, key):
    """S: the largest gap between the reference's own builds, over both feeds."""
    builds = ["_sum4"] + (["_rot64"] if g["mode"] in ROTATOR else [])
    return max(gap(g[f"{feed}_{key}"], g[f"{feed}_{key}{b}"]) for feed in FEEDS for b in builds)


def value_bar(g, key="y"):
    s = own_gap(g, key)
    top = max(float(np.abs(g[f"{feed}_{key}"]).max()) for feed in FEEDS)
    return s, 16 * max(s, 4 * float(EPS32) * top)


def ops_of(g, feed):
    return str(g[f"ops_{feed}"]).split(",")


def dev_per_output(g, feed):
    """The deviation (rad / sample) in force at every output of the feed."""
    p = g["params"]
    dev = 2 * np.pi * (p[1] / 2.0) / p[0] if g["mode"] == "fm" else p[-1]
    out, call = [], 0
    for op in ops_of(g, feed):
        if op[0] == "v":
            dev = float(op[1:])
        elif op[0].isdigit():
            out.append(np.full(int(g[f"{feed}_counts"][call]), dev))
            call += 1
    return np.concatenate(out)


def fm_taps(g):
    fs, bw, lp, hp = g["params"]
    return oracle.band_pass(300.0, bw / 2.0, 100.0, fs) if lp and hp else oracle.low_pass(bw / 2.0, (bw / 2.0) * 0.1, fs)


def bars(g, feed):
    """(S, the value bar, the bar of every output of `feed`)."""
    mode = g["mode"]
    if mode == "quad":
        return 0.0, 0.0, ATAN_BAR / dev_per_output(g, feed)
    if mode == "ddcfm":
        s, bar_fir = value_bar(g, "z")
        zmin = min(float(np.abs(g[f"{f}_z"]).min()) for f in FEEDS)
        return s, bar_fir, (2 * bar_fir / zmin + ATAN_BAR) / dev_per_output(g, feed)
    s, bar = value_bar(g)
    if mode == "fm":
        return s, bar, float(np.abs(fm_taps(g)).sum()) * ATAN_BAR / dev_per_output(g, feed) + bar
    return s, bar, np.full(len(g[f"{feed}_y"]), bar)


# ------------------------------------------------------------------ the blocks under test
class OracleDDC:
    """oracle.Xlator -> oracle.FIR, as the reference's two blocks (the oracle has no fused handle without the demodulator)."""

    def __init__(self, w, taps, decim):
        self.x, self.f = oracle.Xlator(w), oracle.FIR(taps, decim)
        self.set_taps, self.set_decimation = self.f.set_taps, self.f.set_decimation

    def process(self, x):
        return self.f.process(self.x.process(x))

    def reset(self):
        self.x.reset()
        self.f.reset()


def make_block(lib, g):
    mode, p, taps = g["mode"], g["params"], g["taps"]
    cd = not mode.endswith(("_f", "_ff"))
    if mode == "xlator":
        return oracle.Xlator(p[0]) if lib is oracle else dsp.FrequencyXlator(p[0])
    if mode.startswith("fir_"):
        return lib.FIR(taps[0], int(p[0]), complex_data=cd)
    if mode.startswith("pdec_"):
        return lib.PowerDecimator(int(p[0]), complex_data=cd)
    if mode.startswith("poly_"):
        return lib.PolyphaseResampler(int(p[0]), int(p[1]), taps[0], complex_data=cd)
    if mode.startswith("rres_"):
        return lib.RationalResampler(p[0], p[1], complex_data=cd)
    if mode == "rxvfo":
        return lib.RxVFO(*p)
    if mode == "quad":
        return lib.Quadrature(p[0])
    if mode == "fm":
        return lib.FM(p[0], p[1], bool(p[2]), bool(p[3]))
    if mode == "ddc":
        return OracleDDC(p[0], taps[0], int(p[1])) if lib is oracle else dsp.DDC(p[0], taps[0], int(p[1]))
    assert mode == "ddcfm"
    return oracle.DDCFM(p[0], taps[0], int(p[1]), p[2], precise=True) if lib is oracle else dsp.DDCFM(p[0], taps[0], int(p[1]), p[2])


def apply_op(b, op, taps):
    kind, v = op[0], op[1:]
    if kind == "r":
        b.reset()
    elif kind in "wf":
        b.set_offset(float(v))
    elif kind == "d":
        b.set_decimation(int(v))
    elif kind == "t":
        b.set_taps(taps[int(v)])
    else:
        assert kind == "v", op
        b.set_deviation(float(v))


def run_ops(b, x, ops, taps):
    """The outputs of every process() call of the op list, one array per call."""
    out, i = [], 0
    for op in ops:
        if op[0].isdigit():
            out.append(np.array(b.process(x[i:i + int(op)])))
            i += int(op)
        else:
            apply_op(b, op, taps)
    assert i == len(x)
    return out


def against_the_fixture(lib, name):
    g = load(name)
    worst = 0.0
    for feed in FEEDS:
        calls = run_ops(make_block(lib, g), g["x"], ops_of(g, feed), g["taps"])
        want_counts, want = list(g[f"{feed}_counts"]), g[f"{feed}_y"]
        assert [len(c) for c in calls] == want_counts, f"{name} {feed}: per-call output counts"
        y = np.concatenate(calls)
        assert len(y) == len(want) == sum(want_counts)
        s, bar, per_output = bars(g, feed)
        if np.iscomplexobj(y):
            d = np.maximum(np.abs(y.real.astype(np.float64) - want.real), np.abs(y.imag.astype(np.float64) - want.imag))
        else:
            d = np.abs(y.astype(np.float64) - want)
        k = int(np.argmax(d - per_output))
        print(f"{name} {feed}: S {s:.3e}, value bar {bar:.3e}, {lib.__name__.split('.')[-1]} gap {d.max():.3e} "
              f"(worst against its bar at output {k}: {d[k]:.3e} / {per_output[k]:.3e})")
        write_report("ref_pin_chain", {"case": name, "feed": feed, "S": s, "bar": bar, "outputs": len(y),
                                       ("oracle_gap" if lib is oracle else "device_gap"): float(d.max()),
                                       "worst_over_bar": float((d / per_output).max())})
        worst = max(worst, float((d / per_output).max()))
        assert np.all(d <= per_output), f"{name} {feed}: output {k} is {d[k]:.3e} from the reference, bar {per_output[k]:.3e}"
        if g["mode"] == "ddcfm":
            fir_stage_against_the_fixture(lib, g, feed, bar)
    return worst


def fir_stage_against_the_fixture(lib, g, feed, bar_fir):
    """The ddcfm case's FIR-stage output z, which the quadrature bar rests on: the same ops (setDeviation apart)
    through the chain without the demodulator, within the value bar on z."""
    p, taps = g["params"], g["taps"]
    blk = OracleDDC(p[0], taps[0], int(p[1])) if lib is oracle else dsp.DDC(p[0], taps[0], int(p[1]))
    calls = run_ops(blk, g["x"], [op for op in ops_of(g, feed) if op[0] != "v"], taps)
    assert [len(c) for c in calls] == list(g[f"{feed}_counts"]), f"ddcfm {feed}: FIR-stage output counts"
    d = gap(np.concatenate(calls), g[f"{feed}_z"])
    print(f"ddcfm {feed}: FIR stage to reference {d:.3e}, bar {bar_fir:.3e}")
    write_report("ref_pin_chain", {"case": "ddcfm_fir_stage", "feed": feed, "bar": bar_fir,
                                   ("oracle_gap" if lib is oracle else "device_gap"): d})
    assert d <= bar_fir


# ------------------------------------------------------------------ conditions on the fixtures
@pytest.mark.parametrize("name", CASES)
def test_fixture_meets_the_conditions(name):
    g = load(name)
    x, mode = g["x"], g["mode"]
    rms = float(np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2)))
    for feed in FEEDS:
        ops = ops_of(g, feed)
        n_calls = sum(op[0].isdigit() for op in ops)
        assert sum(int(op) for op in ops if op[0].isdigit()) == len(x)
        for b in ("", "_sum4", "_rot64"):
            assert len(g[f"{feed}_counts{b}"]) == n_calls
            assert np.array_equal(g[f"{feed}_counts{b}"], g[f"{feed}_counts"]), f"build {b}: other counts"
            assert len(g[f"{feed}_y{b}"]) == int(g[f"{feed}_counts"].sum())
        assert np.isfinite(g[f"{feed}_y"].view(np.float32)).all()
    assert int(g["whole_counts"].sum()) == int(g["cut_counts"].sum())
    # the cut feed holds calls of 0 and 1 and the setters sit mid-stream
    cut = ops_of(g, "cut")
    assert "0" in cut and "1" in cut and not cut[-1].isalpha() and cut[0].isdigit()
    s, bar = (0.0, 0.0) if mode == "quad" else value_bar(g, "z" if mode == "ddcfm" else "y")
    write_report("ref_pin_chain", {"case": name, "S": s, "bar": bar, "rms_x": rms})
    if name in RANDOM_TAPS:
        hmin = min(float(np.abs(t).min()) for t in g["taps"])
        print(f"{name}: S {s:.3e}, bar {bar:.3e}, smallest |h| rms(x) {hmin * rms:.3e}")
        assert hmin * rms >= 64 * bar, f"a tap of {hmin:.3e} lies within 64 bars ({bar:.3e}) at rms(x) {rms:.3e}"
    if mode in ("xlator", "rxvfo"):
        w = g["params"][0] if mode == "xlator" else -2 * np.pi * g["params"][3] / g["params"][0]
        steps = 0
        for op in ops_of(g, "whole"):
            if op[0] in "wf":
                w2 = float(op[1:]) if mode == "xlator" else -2 * np.pi * float(op[1:]) / g["params"][0]
                assert abs(w2 - w) * rms >= 1000 * bar, f"the retune {op} moves the output by less than 1000 bars"
                w, steps = w2, steps + 1
        assert steps == 1
    if mode == "ddcfm":
        zmin = min(float(np.abs(g[f"{f}_z"]).min()) for f in FEEDS)
        print(f"ddcfm: min|z| {zmin:.3f}")
        assert zmin >= 0.25
        for feed in FEEDS:
            for b in ("_sum4", "_rot64"):
                assert len(g[f"{feed}_z{b}"]) == len(g[f"{feed}_z"])


def test_fir_walk_selects_every_family():
    """FirBlock::select_kernel's rules (blocks.hip) restated on the walk's segments: the matrix-core tiles, the
    row kernel at 8 and at 5 taps per phase, the phase-split tiles and the tile kernel, each entered from
    another family's history."""
    g = load("fir_walk")

    def family(ntaps, D):
        qr = (ntaps + D - 1) // D
        pow2 = D & (D - 1) == 0 and qr <= 32
        if D == 32 and 2 <= qr <= 8:
            return f"rows{qr}"
        if pow2 and D <= 8 and qr >= 16:
            return "mfma"
        return "mfma_ps" if pow2 and 4 <= D <= 32 else "tile"

    ntaps, D, seen, pending = len(g["taps"][0]), int(g["params"][0]), [], True
    for op in ops_of(g, "whole"):
        if op[0] == "t":
            ntaps, pending = len(g["taps"][int(op[1:])]), True
        elif op[0] == "d":
            D, pending = int(op[1:]), True
        elif op[0].isdigit() and pending:
            seen.append(family(ntaps, D))
            pending = False
    assert seen == ["mfma", "rows8", "rows5", "mfma_ps", "tile", "mfma"]


# ------------------------------------------------------------------ the oracle and the device against the fixtures
@pytest.mark.parametrize("name", CASES)
def test_oracle_is_the_reference(name):
    against_the_fixture(oracle, name)


def test_oracle_fp32_path_takes_the_setters():
    """The oracle's fp32 mode (the CPU baseline: the rotator recurrence itself, 8-lane sums) over the RxVFO cases'
    ops: set_offset has to reach its rotator's increment and reset its phasor. Counts as the reference's,
    values within the suite's RxVFO cascade bar (5e-5, test_gpu_parity.py) of it."""
    for name in ("rxvfo_d64", "rxvfo_poly"):
        g = load(name)
        calls = run_ops(oracle.RxVFO(*g["params"], precise=False), g["x"], ops_of(g, "cut"), g["taps"])
        assert [len(c) for c in calls] == list(g["cut_counts"])
        assert_close_c(np.concatenate(calls), g["cut_y"], 5e-5, f"oracle fp32 {name}")


@gpu
@pytest.mark.parametrize("name", CASES)
def test_device_is_the_reference(name):
    against_the_fixture(dsp, name)


# ------------------------------------------------------------------ against the pinned oracle, at the host's other paths
@gpu
def test_rxvfo_big_calls_with_retune_and_reset_vs_oracle():
    """The C5 shape past kTailMaxIn (1,200,000 samples: 37,500 first-stage outputs), at a reference block
    (307,200) and in a short call, set_offset and reset between the calls: counts equal the oracle's, every
    output within test_gpu_parity.py's RxVFO bar."""
    rng = np.random.default_rng(0x5EED19)
    fs = 61.44e6
    g, o = dsp.RxVFO(fs, 240000, 200000, 2.5e6), oracle.RxVFO(fs, 240000, 200000, 2.5e6)
    x = iq(rng, 1200000)
    steps = [1200000, ("set_offset", -1.5e6), 307200, 999, 1200000, ("reset",), 999, 307200, ("set_offset", 7e5), 1200000, 307200]
    worst = 0.0
    for k, st in enumerate(steps):
        if isinstance(st, tuple):
            for b in (g, o):
                getattr(b, st[0])(*st[1:])
            continue
        xs = x[(k * 7919) % 1000:][:st] if st < len(x) else x
        yg, yo = g.process(xs), o.process(xs)
        assert len(yg) == len(yo), f"step {k}: {len(yg)} outputs, the oracle {len(yo)}"
        if len(yo):
            worst = max(worst, assert_close_c(yg, yo, 5e-5, f"rxvfo step {k} ({st} samples)"))
    write_report("ref_pin_chain", {"case": "rxvfo_c5_big_calls", "device_to_oracle": float(worst), "bar": 5e-5})


@gpu
def test_fir_walk_at_200k_per_segment_vs_oracle():
    """The fixture's FIR walk (every kernel family entered from another's history, offset 0 after each setter)
    at 200,000 samples per segment plus an odd remainder, so each segment ends inside a decimation period."""
    f = load("fir_walk")
    rng = np.random.default_rng(0xF1219)
    g, o = dsp.FIR(f["taps"][0], int(f["params"][0])), oracle.FIR(f["taps"][0], int(f["params"][0]))
    taps, worst = f["taps"][0], 0.0
    for k, op in enumerate(ops_of(f, "whole")):
        if op[0].isdigit():
            x = iq(rng, 200000 + int(op) % 37)
            yg, yo = g.process(x), o.process(x)
            assert len(yg) == len(yo), f"op {k}: {len(yg)} outputs, the oracle {len(yo)}"
            worst = max(worst, assert_close_c(yg, yo, fir_atol(taps, x), f"FIR walk, op {k}") / fir_atol(taps, x))
        else:
            if op[0] == "t":
                taps = f["taps"][int(op[1:])]
            for b in (g, o):
                apply_op(b, op, f["taps"])
    write_report("ref_pin_chain", {"case": "fir_walk_200k", "worst_over_fir_atol": float(worst)})


# --------------------------------------------------------------- live probe
@pytest.mark.skipif(not have_reference(), reason="reference tree not mounted (GPU box): the committed fixtures cover it")
def test_live_reference_probe_reproduces_the_fixtures():
    assert_live_probe_reproduces("ref_chain_", "chain_fixtures")
