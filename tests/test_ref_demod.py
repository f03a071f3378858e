"""The analogue demodulators pinned to the REFERENCE's own headers, setters and reset included:
tests/golden/ref_demod_*.npz hold what oracle/_ref/ref_blocks -- demod/am.h, ssb.h, cw.h and broadcast_fm.h
compiled over oracle/ref_standins.cpp -- computes for demod::AM, SSB, CW (float and stereo_t) and BroadcastFM
(tools/gen_ref_fixtures.py demod_cases). Every case is an op list: sample counts (process() calls) and,
mid-stream, `r` reset (AM, BroadcastFM), `g<x>` setAGCGain, `e<0|1>` setAGCEnabled (SSB, CW), `a<att>x<dec>`
setAGCAttack + setAGCDecay, `b<rate>` AM::setDCBlockRate, `w<hz>` CW::setTone and `R<0|1>`
BroadcastFM::setRDSOut. It is fed twice: every segment whole, and every segment in calls of 1, 0, a count below
the block's history, 7, 0, 129, 1024, 1025 (BroadcastFM: and 152, 153, 154, around its delay of 153) and the rest
in two. Besides the output the AM cases record the low-pass filter's input of every call, the BroadcastFM cases
every call's RDS count and samples. Four builds of the reference are used: VOLK's dot products summed in
ascending order (whose outputs are stored), in the order of a 4-lane SIMD kernel (_sum4), ascending with the
rotator's phase in fp64 (_rot64: SSB, CW, the RDS branch) and ascending with cosf / sinf / atan2f evaluated in
fp64 and rounded once (_trig64: BroadcastFM; built through the forced-include header oracle/ref_trig64.h, which
compiled cleanly over <cmath>, so no restated trig gap is used). Of the three other builds the fixtures keep the
per-call counts and the largest distance from the ascending build per feed (the outputs themselves would take the
files past the size limit).

Bars, for the C oracle (precise mode, on the CPU), the dsp.* blocks and the banks (on the device):
* Counts: exact per call, the RDS count of every call included.
* AM's low-pass input: equal value for value (the AGC, the magnitude sqrtf(re re + im im) without contraction
  and the DC blocker are recurrences or single roundings in the reference's order).
* AM's output, SSB and CW with the AGC on, BroadcastFM stereo per channel, the RDS samples: within
  16 max(S, 4 eps32 max|y|) of the ascending build, S the largest gap between the ascending build and _sum4
  (AM), _sum4 and _rot64 (SSB, CW), _sum4 and _trig64 (BroadcastFM stereo), all of them (RDS), over both feeds.
* SSB and CW with the AGC off (a 1e7 limiter; CW after `g1e7`, its own initial gain being 1): outputs whose
  reference magnitude is at the clip (10 for SSB, 1 for CW) within 16 eps32 clip, which fixes sign and value; the
  rest at the bar above. At least 99 % of the reference's samples are clipped in every build.
* BroadcastFM mono: sum|h| ATAN_BAR / dev plus the value bar (S from _sum4), FM's bar of test_ref_chain.py;
  l equals r bit for bit.
Conditions on the fixtures are asserted on the CPU (test_fixture_meets_the_conditions and the tests after it): equal
counts in all builds, every output compared, every op of a case moves the 2,000 outputs after it by at least 1000
bars against a run without it (each case holds only ops that act in it: an enabled AGC overwrites a set gain at the
next sample, a disabled one ignores attack and decay), at least 99 % clipped where the AGC is off, the stereo
decoding real (test_stereo_decoding_is_real, which also says why bfm_stereo_std exists), and the two reset cases:
BroadcastFM::reset() leaves the RDS branch's xlator phase and resampler history (83 RDS samples after the reset
where a fresh branch gives 84, 2e-3 apart) and AM::reset() leaves the low-pass filter's history (the 363 outputs
after it lie 4e-2 from a zeroed history's). Both were what the reference does and not what the device did; the
device, the banks and the drop-in now follow the reference. am_reset holds the reset alone, so that a bank, which has
no attack / decay or DC-rate setter and runs a case only up to the first op it lacks, reaches it.
One mutation of the issue's list cannot be caught by any test of the audio: the conjugate ahead of the two complex
multiplies. The delayed MPX is real (imaginary part exactly 0) and only the real part of the product is kept, and
Re(x p p) = Re(x conj(p) conj(p)) for real x, operation by operation, so the result is the same bit for bit.
Recorded: profiles/r22/ref_pin_demod.json.
"""
import glob
import os

import numpy as np
import pytest

import oracle
from sdrpp_amd import dsp
from _util import EPS32, GOLDEN, assert_live_probe_reproduces, have_reference, write_report

gpu = pytest.mark.gpu
FEEDS = ("whole", "cut")
ATAN_BAR = 8 * float(np.spacing(np.float32(np.pi)))
CASES = ["am_audio", "am_carrier", "am_off", "am_reset", "am_stereo", "bfm_mono", "bfm_mono_rds", "bfm_ops", "bfm_stereo_lp",
         "bfm_stereo_raw", "bfm_stereo_rds", "bfm_stereo_std", "cw", "cw_agc_off", "cw_stereo", "ssb_agc_off", "ssb_dsb",
         "ssb_lsb", "ssb_stereo", "ssb_usb"]
BFM_DELAY = 153
SETTLED = 12000                 # BroadcastFM: outputs after which the 1 kHz amplitudes are read (50 ms)
MOVED_WINDOW = 2000
_cache = {}


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, f"ref_demod_{name}.npz")) as f:
            g = {k: f[k] for k in f.files}
        g["x"] = from_i16(g["xi16"])
        g["mode"], g["builds"] = str(g["mode"]), [str(b) for b in g["builds"]]
        g["x"].setflags(write=False)
        _cache[name] = g
    return _cache[name]


def from_i16(k):
    x = (np.asarray(k, np.float32) / np.float32(32768.0)).astype(np.float32)
    return np.ascontiguousarray(x).view(np.complex64)[:, 0]


def test_the_case_list_is_the_fixtures():
    on_disk = {os.path.basename(p)[len("ref_demod_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "ref_demod_*.npz"))}
    assert on_disk == set(CASES)


def parts(a):
    """float32 view: the components of complex64 / stereo pairs side by side."""
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.float32)


def dist(a, b):
    a, b = parts(a).astype(np.float64), parts(b).astype(np.float64)
    assert a.shape == b.shape
    return np.abs(a - b)


def ops_of(g, feed):
    return str(g[f"ops_{feed}"]).split(",")


def family(g):
    return g["mode"].split("_")[0]


def agc_off(g):
    return family(g) in ("ssb", "cw") and "clipped" in g


def own_gap(g, stream, builds=None):
    """S: the largest gap between the ascending build and the others, over both feeds."""
    return max(float(g[f"gap_{stream}{b}"].max()) for b in (builds or g["builds"]))


def value_bar(g, stream="y", builds=None):
    s = own_gap(g, stream, builds)
    top = max(float(np.abs(parts(g[f"{feed}_{stream}"])).max(initial=0.0)) for feed in FEEDS)
    return s, 16 * max(s, 4 * float(EPS32) * top)


def clip_of(g):
    return 10.0 if family(g) == "ssb" else 1.0


def clip_bar(g):
    return 16 * float(EPS32) * clip_of(g)


def bfm_mono_bar(g):
    dev_hz, fs, _, lp, _ = g["params"]
    s, bar = value_bar(g, "y", ["_sum4"])
    h = float(np.abs(oracle.low_pass(15000.0, 4000.0, fs)).sum()) if lp else 1.0
    return s, h * ATAN_BAR / (2 * np.pi * dev_hz / fs) + (bar if lp else 0.0)


def bars(g, feed):
    """(S, the bar of every float32 component of the feed's output)."""
    want = parts(g[f"{feed}_y"])
    if family(g) == "bfm" and not g["params"][2]:
        s, bar = bfm_mono_bar(g)
        return s, np.full(len(want), bar)
    s, bar = value_bar(g)
    per = np.full(len(want), bar)
    if agc_off(g):
        per[np.abs(want) >= clip_of(g) * (1 - 1e-6)] = clip_bar(g)
    return s, per


def moved_bar(g):
    """The bar that a setter's effect is measured against: where the AGC is off, the clipped samples' (the general
    bar there is the limiter's gain times the rotator's rounding, which no setter could exceed 1000 times)."""
    if agc_off(g):
        return clip_bar(g)
    if family(g) == "bfm" and not g["params"][2]:
        return bfm_mono_bar(g)[1]
    return value_bar(g)[1]


# ------------------------------------------------------------------ the blocks under test
def make_block(lib, g, **kw):
    fam, p, st = family(g), g["params"], g["mode"].endswith("_s")
    if fam == "am":
        if lib is oracle:
            return oracle.AM(int(p[0]), *p[1:], precise=True, stereo=st, **kw)
        b = dsp.AM(int(p[0]), *p[1:], stereo=st)
        if kw.get("unit_low_pass"):
            b.set_low_pass_taps([1.0])
        return b
    if fam == "ssb":
        return lib.SSB(int(p[0]), p[1], p[2], bool(p[3]), p[4], p[5], stereo=st)
    if fam == "cw":
        return lib.CW(p[0], bool(p[1]), p[2], p[3], p[4], stereo=st)
    assert fam == "bfm"
    if lib is oracle:
        return oracle.BroadcastFMStereo(p[0], p[1], bool(p[2]), bool(p[3]), precise=True, rds=bool(p[4]))
    return dsp.BroadcastFM(p[0], p[1], bool(p[3]), stereo=bool(p[2]), rds=bool(p[4]))


def apply_op(b, op):
    kind, v = op[0], op[1:]
    if kind == "r":
        b.reset()
    elif kind == "g":
        b.set_agc_gain(float(v))
    elif kind == "e":
        b.set_agc_enabled(int(v))
    elif kind == "a":
        b.set_agc_attack_decay(*map(float, v.split("x")))
    elif kind == "b":
        b.set_dc_block_rate(float(v))
    elif kind == "w":
        b.set_tone(float(v))
    else:
        assert kind == "R", op
        if isinstance(b, oracle.BroadcastFMStereo):
            b.set_rds(int(v))
        else:
            b.set_rds_out(int(v))          # sdrgpu_broadcast_fm_set_rds, then sdrgpu_block_reset


def run_ops(b, x, ops, rds=False):
    """The outputs (and RDS samples) of every process() call of the op list, one array per call."""
    out, tail, i = [], [], 0
    for op in ops:
        if op[0].isdigit():
            out.append(np.array(b.process(x[i:i + int(op)])))
            if rds:                        # (a block made without the RDS branch has no RDS output to ask for)
                tail.append(np.array(b.rds_output()) if rds == "on" else np.empty(0, np.complex64))
            i += int(op)
        else:
            apply_op(b, op)
    assert i == len(x)
    return out, tail


def joined(calls, dtype):
    return np.concatenate(calls) if calls else np.empty(0, dtype)


def against_the_fixture(lib, name):
    g = load(name)
    who = "oracle" if lib is oracle else "device"
    for feed in FEEDS:
        ops, is_bfm = ops_of(g, feed), family(g) == "bfm"
        calls, tail = run_ops(make_block(lib, g), g["x"], ops, rds=is_bfm and ("on" if g["params"][4] else "off"))
        want_counts, want = list(g[f"{feed}_counts"]), g[f"{feed}_y"]
        assert [len(c) for c in calls] == want_counts, f"{name} {feed}: per-call output counts"
        y = joined(calls, want.dtype)
        assert len(y) == len(want) == sum(want_counts)
        s, per = bars(g, feed)
        d = dist(y, want)
        k = int(np.argmax(d - per)) if d.size else 0
        rep = {"case": name, "feed": feed, "S": s, "bar": float(per.max()), "outputs": len(y), f"{who}_gap": float(d.max())}
        print(f"{name} {feed}: S {s:.3e}, bar {per.max():.3e}, {who} gap {d.max():.3e} "
              f"(worst against its bar at component {k}: {d[k]:.3e} / {per[k]:.3e})")
        if is_bfm:
            s_rds, bar_rds = value_bar(g, "rds")
            got_counts = [len(t) for t in tail]
            rds = joined(tail, np.complex64)
            d_rds = dist(rds, g[f"{feed}_rds"]) if got_counts == list(g[f"{feed}_rds_counts"]) else None
            rep.update({"S_rds": s_rds, "bar_rds": bar_rds, "rds_samples": len(rds),
                        f"{who}_gap_rds": float(d_rds.max()) if d_rds is not None and d_rds.size else 0.0})
            print(f"{name} {feed}: RDS S {s_rds:.3e}, bar {bar_rds:.3e}, {who} gap {rep[f'{who}_gap_rds']:.3e}, {len(rds)} samples")
        write_report("ref_pin_demod", rep)
        assert np.all(d <= per), f"{name} {feed}: component {k} is {d[k]:.3e} from the reference, bar {per[k]:.3e}"
        if is_bfm:
            assert got_counts == list(g[f"{feed}_rds_counts"]), f"{name} {feed}: per-call RDS counts"
            assert np.all(d_rds <= bar_rds), f"{name} {feed}: an RDS sample is {d_rds.max():.3e} from the reference, bar {bar_rds:.3e}"
            if not g["params"][2]:
                assert np.array_equal(y["l"].view(np.uint32), y["r"].view(np.uint32)), "mono: l is not r"
        if family(g) == "am":
            zc, _ = run_ops(make_block(lib, g, unit_low_pass=True), g["x"], ops)
            z = joined(zc, want.dtype)
            z = z["l"] if g["mode"].endswith("_s") else z
            assert [len(c) for c in zc] == want_counts
            same = np.array_equal(z, g[f"{feed}_z"])
            write_report("ref_pin_demod", {"case": name + "_lowpass_input", "feed": feed, f"{who}_equal": bool(same)})
            assert same, f"{name} {feed}: the low-pass filter's input differs from the reference's, first at " \
                         f"{int(np.argmax(z != g[f'{feed}_z']))}, by up to {dist(z, g[f'{feed}_z']).max():.3e}"


# ------------------------------------------------------------------ conditions on the fixtures
def tone_amplitude(y, hz, fs):
    t = np.arange(len(y))
    return 2 * abs(np.mean(y.astype(np.float64) * np.exp(-2j * np.pi * hz * t / fs)))


@pytest.mark.parametrize("name", CASES)
def test_fixture_meets_the_conditions(name):
    g = load(name)
    x, fam = g["x"], family(g)
    for feed in FEEDS:
        ops = ops_of(g, feed)
        n_calls = sum(op[0].isdigit() for op in ops)
        assert sum(int(op) for op in ops if op[0].isdigit()) == len(x)
        counts = g[f"{feed}_counts"]
        assert len(counts) == n_calls and len(g[f"{feed}_y"]) == int(counts.sum())
        for b in g["builds"]:
            assert np.array_equal(g[f"{feed}_counts{b}"], counts), f"build {b}: other counts"
            assert np.isfinite(g[f"gap_y{b}"]).all(), f"build {b}: another output length"
            if fam == "bfm":
                assert np.array_equal(g[f"{feed}_rds_counts{b}"], g[f"{feed}_rds_counts"]), f"build {b}: other RDS counts"
                assert np.isfinite(g[f"gap_rds{b}"]).all()
        assert np.isfinite(parts(g[f"{feed}_y"])).all()
        if fam == "am":
            assert len(g[f"{feed}_z"]) == int(counts.sum())
        if fam == "bfm":
            assert len(g[f"{feed}_rds_counts"]) == n_calls and len(g[f"{feed}_rds"]) == int(g[f"{feed}_rds_counts"].sum())
            assert (len(g[f"{feed}_rds"]) > 400) == bool(g["params"][4])
    cut = ops_of(g, "cut")
    assert "0" in cut and "1" in cut and cut[-1][0].isdigit()
    if fam == "bfm":
        ntaps = len(oracle.band_pass(18750.0, 19250.0, 3000.0, g["params"][1], True, complex_taps=True))
        assert (ntaps - 1) // 2 + 1 == BFM_DELAY
        assert all(str(c) in cut for c in (BFM_DELAY - 1, BFM_DELAY, BFM_DELAY + 1))
    builds = {"am": ["_sum4"], "ssb": ["_sum4", "_rot64"], "cw": ["_sum4", "_rot64"]}.get(fam)
    if fam == "bfm":
        builds = ["_sum4", "_trig64"] + (["_rot64"] if g["params"][4] else [])
    assert g["builds"] == builds
    s, bar = value_bar(g)
    write_report("ref_pin_demod", {"case": name, "S": s, "bar": bar, "moved": g["moved"].tolist(), "moved_bar": moved_bar(g)})
    # every setter moves the output
    whole = ops_of(g, "whole")
    assert len(g["moved"]) == sum(not op[0].isdigit() for op in whole)
    for op, at, moved in zip([op for op in whole if not op[0].isdigit()], g["op_at"], g["moved"]):
        print(f"{name}: {op} at output {at} moves the next {MOVED_WINDOW} outputs by {moved:.3e}, bar {moved_bar(g):.3e}")
        assert moved >= 1000 * moved_bar(g), f"the op {op} moves the output by less than 1000 bars"
    if agc_off(g):
        print(f"{name}: {float(g['clipped']):.4%} of the reference's outputs are at the clip in the build with the fewest")
        assert float(g["clipped"]) >= 0.99


def test_stereo_decoding_is_real():
    """The inputs carry 1 kHz on the left channel only. In every stereo case both channels' 1 kHz amplitudes after the
    settling prefix are at least 1000 bars, so that a wrong delay, a missing 2x, a missing conjugate or swapped
    channels cannot fit inside the bar. That r holds less than 5 % of l's amplitude is asserted on bfm_stereo_std,
    whose pilot and subcarrier have the broadcast standard's phase relation (sin th, sin 2 th): l 0.6556, r 0.0194.
    On fm_stereo_iq's multiplex (cos th, cos 2 th: bfm_stereo_lp and the other cases) the reference's own decoder does
    not separate: its regenerated subcarrier stands 109.5 degrees from the sent one, 2 (L - R) comes out times
    cos(109.5 deg) = -1 / 3, and l is 0.2248, r 0.4502 (0.3375 -+ 0.1125). That is the reference's answer to that
    input, so there the side amplitude |l - r| / 2 is held to that known answer instead."""
    for name in ("bfm_stereo_std", "bfm_stereo_lp"):
        g = load(name)
        y, fs = g["whole_y"][SETTLED:], g["params"][1]
        l, r = tone_amplitude(y.real, 1000.0, fs), tone_amplitude(y.imag, 1000.0, fs)
        mid, side = tone_amplitude((y.real + y.imag) / 2, 1000.0, fs), tone_amplitude((y.real - y.imag) / 2, 1000.0, fs)
        bar = value_bar(g)[1]
        print(f"{name} 1 kHz: l {l:.4f}, r {r:.4f} ({r / l:.2%}), (l + r) / 2 {mid:.4f}, (l - r) / 2 {side:.4f}, bar {bar:.3e}")
        write_report("ref_pin_demod", {"case": name + "_separation", "l_1khz": l, "r_1khz": r, "mid": mid, "side": side, "bar": bar})
        assert l >= 1000 * bar and r >= 1000 * bar
        assert abs(mid - 0.3375) <= 0.01 * 0.3375           # 0.45 x 75 kHz / 100 kHz
        if name == "bfm_stereo_std":
            assert r < 0.05 * l
        else:
            assert abs(side - 0.3375 / 3) <= 0.01 * 0.3375


def test_bfm_reset_keeps_the_rds_branch():
    """After `r` in bfm_ops the reference's RDS samples are not what a fresh RDS branch gives (the pinned oracle,
    new, fed the samples after the reset: every state that reset() restores is then as after reset(), the
    xlator's phase and the resampler's history are zero instead): the count differs or a sample does by 1000 S_rds."""
    g = load("bfm_ops")
    ops = ops_of(g, "whole")
    assert ops[1] == "r"
    n0, n1 = int(ops[0]), int(ops[2])
    first = int(g["whole_rds_counts"][0])
    kept = g["whole_rds"][first:first + int(g["whole_rds_counts"][1])]
    fresh = make_block(oracle, g)
    fresh.process(g["x"][n0:n0 + n1])
    new = fresh.rds_output()
    s_rds = own_gap(g, "rds")
    m = min(len(kept), len(new))
    d = float(dist(kept[:m], new[:m]).max())
    print(f"RDS after reset: {len(kept)} samples, a fresh branch {len(new)}, apart by {d:.3e}, S_rds {s_rds:.3e}")
    write_report("ref_pin_demod", {"case": "bfm_ops_reset_rds", "kept": len(kept), "fresh": len(new), "apart": d, "S_rds": s_rds})
    assert len(kept) != len(new) or d >= 1000 * s_rds


@pytest.mark.parametrize("name", ["am_audio", "am_carrier", "am_off", "am_reset", "am_stereo"])
def test_am_reset_keeps_the_low_pass_history(name):
    """After `r` in the AM cases the first ntaps - 1 outputs are not what a zeroed low-pass history gives (the pinned
    oracle, new, given the setters before the reset and fed the samples after it), by at least 1000 bars."""
    g = load(name)
    ops = ops_of(g, "whole")
    k = ops.index("r")
    done = sum(int(op) for op in ops[:k] if op[0].isdigit())
    fresh = make_block(oracle, g)
    for op in ops[:k]:
        if op[0] in "ab":
            apply_op(fresh, op)
    ntaps = len(oracle.low_pass(g["params"][1] / 2.0, (g["params"][1] / 2.0) * 0.1, g["params"][5]))
    zeroed = fresh.process(g["x"][done:done + ntaps - 1])
    d = float(dist(zeroed, g["whole_y"][done:done + ntaps - 1]).max())
    bar = value_bar(g)[1]
    print(f"{name}: the {ntaps - 1} outputs after the reset lie {d:.3e} from a zeroed history's, bar {bar:.3e}")
    write_report("ref_pin_demod", {"case": name + "_reset_lowpass", "apart": d, "bar": bar})
    assert d >= 1000 * bar


# ------------------------------------------------------------------ the oracle and the device against the fixtures
@pytest.mark.parametrize("name", CASES)
def test_oracle_is_the_reference(name):
    against_the_fixture(oracle, name)


@gpu
@pytest.mark.parametrize("name", CASES)
def test_device_is_the_reference(name):
    against_the_fixture(dsp, name)


# ------------------------------------------------------------------ the banks
def bank_of(g, S):
    fam, p = family(g), g["params"]
    if fam == "am":
        return dsp.BankAM(S, int(p[0]), *p[1:])
    if fam == "ssb":
        return dsp.BankSSB(S, int(p[0]), p[1], p[2], bool(p[3]), p[4], p[5])
    if fam == "cw":
        return dsp.BankCW(S, p[0], bool(p[1]), p[2], p[3], p[4])
    return dsp.BankBroadcastFM(S, p[0], p[1], bool(p[3]), bool(p[2]))


def bank_op(b, g, op):
    """The op on the bank; False where the bank has no such setter."""
    kind, v = op[0], op[1:]
    if kind == "r" and family(g) in ("am", "bfm"):
        b.reset()
    elif kind == "g":
        b.set_agc_gain(float(v))
    elif kind == "w":
        b.set_offset(2.0 * np.pi * (float(v) / g["params"][4]))      # CW::setTone: hzToRads(tone, samplerate)
    else:
        return False
    return True


def bank_against_the_fixture(name, S=3):
    """The case through a bank of S = 3 streams, the fixture's input in column 1 and independent noise in columns 0
    and 2, up to the first op the bank has no setter for: column 1 meets the fixture's counts and bars, and is bit
    for bit the same with other neighbours."""
    g = load(name)
    x = g["x"]
    for feed in FEEDS:
        runs = []
        for seed in (1, 2):
            rng = np.random.default_rng(0xB0 + seed)
            X = (0.3 * (rng.uniform(-1, 1, (len(x), S)) + 1j * rng.uniform(-1, 1, (len(x), S)))).astype(np.complex64)
            X[:, 1] = x
            b, out, i = bank_of(g, S), [], 0
            for op in ops_of(g, feed):
                if op[0].isdigit():
                    out.append(np.array(b.process(X[i:i + int(op)])[:, 1]))
                    i += int(op)
                elif not bank_op(b, g, op):
                    break
            runs.append(out)
        calls = runs[0]
        want_counts = list(g[f"{feed}_counts"][:len(calls)])
        assert calls and [len(c) for c in calls] == want_counts, f"{name} {feed}: per-call output counts"
        y = np.concatenate(calls)
        want = g[f"{feed}_y"][:len(y)]
        s, per = bars(g, feed)
        per = per[:len(parts(want))]
        d = dist(y, want)
        k = int(np.argmax(d - per))
        print(f"bank {name} {feed}: {len(calls)} calls, {len(y)} outputs, S {s:.3e}, bar {per.max():.3e}, gap {d.max():.3e}")
        write_report("ref_pin_demod", {"case": "bank_" + name, "feed": feed, "S": s, "bar": float(per.max()), "calls": len(calls),
                                       "outputs": len(y), "device_gap": float(d.max())})
        assert np.all(d <= per), f"bank {name} {feed}: component {k} is {d[k]:.3e} from the reference, bar {per[k]:.3e}"
        assert np.array_equal(parts(y).view(np.uint32), parts(np.concatenate(runs[1])).view(np.uint32)), "the neighbours leak"


@gpu
def test_bank_am_is_the_reference():
    for name in ("am_carrier", "am_audio", "am_off", "am_reset"):
        bank_against_the_fixture(name)
    assert len(ops_of(load("am_reset"), "whole")) == 3         # (all of it runs on the bank: the reset is compared)


@gpu
def test_bank_ssb_is_the_reference():
    for name in ("ssb_usb", "ssb_lsb", "ssb_dsb", "ssb_agc_off"):
        bank_against_the_fixture(name)


@gpu
def test_bank_cw_is_the_reference():
    for name in ("cw", "cw_agc_off"):
        bank_against_the_fixture(name)


@gpu
def test_bank_broadcast_fm_is_the_reference():
    for name in ("bfm_stereo_lp", "bfm_stereo_std", "bfm_stereo_raw", "bfm_mono", "bfm_ops"):
        bank_against_the_fixture(name)


# ------------------------------------------------------------------ against the pinned oracle, past the fixtures' sizes
@gpu
def test_broadcast_fm_stereo_one_call_of_40000_vs_oracle():
    """A call longer than 32,768 samples: 40,000 samples of bfm_stereo_lp's kind of input in one call, against the
    pinned oracle at the 2e-5 of full scale of test_loops.py's test_broadcast_fm_stereo_vs_oracle."""
    from test_loops import fm_stereo_iq
    fs = 240000.0
    x = fm_stereo_iq(40000, fs)
    a = dsp.BroadcastFM(100000, fs, True, stereo=True).process(x)
    b = oracle.BroadcastFMStereo(100000, fs, True, True).process(x)
    assert a.shape == b.shape == (40000,)
    for ch in ("l", "r"):
        err = float(np.abs(a[ch].astype(np.float64) - b[ch]).max())
        write_report("ref_pin_demod", {"case": "bfm_stereo_40000", "channel": ch, "device_to_oracle": err, "bar": 2e-5})
        assert err <= 2e-5 * max(float(np.abs(b[ch]).max()), 1.0), f"{ch}: {err:.3e}"


# --------------------------------------------------------------- live probe
@pytest.mark.skipif(not have_reference(), reason="reference tree not mounted (GPU box): the committed fixtures cover it")
def test_live_reference_probe_reproduces_the_fixtures():
    assert_live_probe_reproduces("ref_demod_", "demod_fixtures")
