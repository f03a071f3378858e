"""The restatements, the C oracle's loops, the host design code and the device kernels pinned to the
REFERENCE's own stateful block headers: tests/golden/ref_blocks_*.npz hold what
oracle/_ref/ref_blocks -- the reference's loop, symbol recovery, IF noise reduction and PSK / GFSK
headers compiled over oracle/ref_standins.cpp's scalar VOLK and fp64-DFT FFTW stand-ins -- computes
on the suite's own signals (tools/gen_ref_fixtures.py), fed in one call and in the cuts
[1, 6, 7, 8, 0, 1023, 1024, 1025, 4097, rest].

Bars:
* FastAGC, MM (every call's count and every output, also after setInterpParams, reset and setOmega),
  slicer, differential decoder, noise blanker, squelch, loop::AGC, DC blocker, de-emphasis -- bit for
  bit: these are recurrences in the reference's own operation order, anything short of identity is a
  misreading. On the CPU for tests/_restated.py and the C oracle, on the device for the kernels.
* Costas -- the bar of test_symsync.py: 16 max(S, 4 eps32 max|y|), S = the restatement's own gap
  between float32 and fp64 trig over 8 seeds. The fixture (glibc cosf / sinf) is one more libm.
* FMIF -- the reference's output must pass test_ifnr.py's fmif_check in the device's place, with at
  most 1 % of the samples undecidable: that pins the bar (scale, the B/2 phase, the first-maximum
  tie-break, the window) to the reference.
* Design code -- dsp.root_raised_cosine, dsp.mm_interp_bank, dsp.fmif_window bit for bit.
* Chains (PSK<2>, PSK<4>, GFSK, the RDS bit chain) -- the reference is built twice, with VOLK's dot
  products summed in ascending order and in the order of a 4-lane SIMD kernel. S_chain = the largest
  gap between the two builds' outputs after the settling prefix the known-answer tests skip (1000
  symbols, 600 for RDS): the reference's own sensitivity to a summation order it does not fix. The
  device must give the ascending build's output count, identical hard decisions (the quadrant for
  PSK, the sign for GFSK, the bits for RDS) and outputs within 16 max(S_chain, 4 eps32 max|y|) over
  that span (16: the margin of the Costas bar, for the same reason -- the device's libm and summation
  order are one more rounding of the same class). Conditions on the inputs, checked here on the CPU:
  both builds give equal counts and identical hard decisions, and no reference symbol lies within the
  bar of a decision boundary, where a deviation the bar allows would flip a decision (the BPSK seed
  is chosen for that: its quadrant hangs on the sign of a noise-only imaginary part).
  One more condition, without which S_chain means nothing: MM picks one of P = 128 interpolator
  branches per symbol, floor(phase x P) (mm.h:111). A symbol whose phase x P sits next to an integer
  takes the neighbouring branch under any last-bit change upstream, its output moves by the step
  between two branches (3e-3 here, 300 times the bar) and the timing loop carries that on. This is
  the reference's own discontinuity: its two builds show it on 5 of 18 BPSK seeds, and a restated
  chain with 4-lane FIR sums shows it on seeds where the two builds happen to agree. So the chain is
  also restated block by block (its output must be the reference's within the bar), with its FIR sums
  in 1 and 4 lanes and its Costas phasor from float32 and fp64 trig. S_u = the largest change of
  phase x P among those four, and every symbol must keep phase x P more than 2 max(S_u, 4 eps32 P)
  from an integer. (2, not 16: phase is carried at the ulp of omega, so phase x P moves in steps of
  2^-14, S_u is 2 to 8 steps, and 2,000 symbols spread over the branch grid leave a smallest
  distance near 1 / 4,000 -- no seed of 180 tried keeps 16 S_u. The device's rounding is none of the
  four restated ones, so a branch change on the device stays possible; it would show as isolated
  symbols off by the branch step, not as a wiring error, which moves every symbol.)
* Squelch counts per object in this project where squelch.h:40 has one static counter per process
  (tests/_restated.py SquelchRef); the fixture runs a single object, so the two cannot differ.
Recorded: profiles/r12/ref_pin.json.
"""
import os

import numpy as np
import pytest

import oracle
import sdrpp_amd
from sdrpp_amd import dsp
from _util import EPS32, GOLDEN, assert_live_probe_reproduces, have_reference, write_report
import _restated as R
from _restated import f32, N, CUTS, same, parts

gpu = pytest.mark.gpu
OM2 = 5000.0 / 1187.5
MM_BASE = (4.0, 2.5e-5, 0.01, 0.01)


def load(name):
    return np.load(os.path.join(GOLDEN, f"ref_blocks_{name}.npz"))


def gap(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if np.iscomplexobj(a):
        return float(max(np.abs(a.real - b.real).max(), np.abs(a.imag - b.imag).max()))
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


def in_calls(block, x, cuts=CUTS):
    """The outputs of `block` fed `x` in calls of `cuts`, one array per call."""
    out, i = [], 0
    for c in cuts:
        out.append(block.process(x[i:i + c]))
        i += c
    assert i == len(x)
    return out


def whole_and_cut(make, x, want, what, want_cut=None, cuts=CUTS):
    """`make()` fed in one call equals `want` bit for bit, and fed in `cuts` equals `want_cut` (`want`
    where the reference itself does not depend on the cuts)."""
    y = make().process(x)
    assert same(np.asarray(y), want), f"{what}: one call differs from the reference"
    z = np.concatenate(in_calls(make(), x, cuts))
    assert same(z, want if want_cut is None else want_cut), f"{what}: the stream in calls differs from the reference"


def cplx(re, im):
    return (re[0] + 1j * im[0]).astype(np.complex64)


def test_fixture_cuts_are_the_suites():
    for name in ("sym", "mm", "costas_a", "costas_b", "ifnr", "loops_a", "loops_b", "chains_a", "chains_b"):
        assert list(load(name)["cuts"]) == CUTS, name


# ------------------------------------------------------------------ FastAGC
class RestatedFastAGC:
    def __init__(self, set_point, max_gain, rate, init_gain, complex_data):
        self.args, self.gain, self.cplx = (set_point, max_gain, rate), f32(init_gain), complex_data

    def process(self, x):
        if not len(x):
            return x.copy()
        xr, xi = parts(x)
        yr, yi, g = R.ref_fast_agc(xr, xi if self.cplx else None, *self.args, self.gain)
        self.gain = g[0]
        return cplx(yr, yi) if self.cplx else yr[0]


def fast_agc_case(complex_data):
    g = load("sym")
    x = g["fastagc_x"] if complex_data else np.ascontiguousarray(g["fastagc_x"].real)
    return x, g["fastagc_y_c" if complex_data else "fastagc_y_f"], tuple(g["fastagc_params"])


@pytest.mark.parametrize("complex_data", [False, True])
def test_fast_agc_restatement_is_the_reference(complex_data):
    x, want, p = fast_agc_case(complex_data)
    assert np.any(want[5000:5100] == 0) and len(want) == N
    whole_and_cut(lambda: RestatedFastAGC(*p, complex_data), x, want, "ref_fast_agc")


@gpu
@pytest.mark.parametrize("complex_data", [False, True])
def test_fast_agc_device_is_the_reference(complex_data):
    x, want, p = fast_agc_case(complex_data)
    whole_and_cut(lambda: dsp.FastAGC(*p, complex_data=complex_data), x, want, "FastAGC")


# ---------------------------------------------- slicer, differential decoder
class Stateless:
    def __init__(self, fn):
        self.process = fn


class RestatedDiff:
    def __init__(self, modulus, init):
        self.modulus, self.last = modulus, init

    def process(self, x):
        if not len(x):
            return x.copy()
        y = R.ref_diff(x, self.modulus, self.last)
        self.last = x[-1]
        return y


def test_slicer_and_differential_decoder_restatements_are_the_reference():
    g = load("sym")
    assert g["slicer_y"].dtype == np.uint8 and 0 < g["slicer_y"].sum() < N
    whole_and_cut(lambda: Stateless(R.ref_slicer), g["slicer_x"], g["slicer_y"], "ref_slicer")
    for m in (2, 4):
        whole_and_cut(lambda: RestatedDiff(m, int(g[f"diff{m}_init"])), g[f"diff{m}_x"], g[f"diff{m}_y"], f"ref_diff {m}")


@gpu
def test_slicer_and_differential_decoder_device_is_the_reference():
    g = load("sym")
    whole_and_cut(dsp.BinarySlicer, g["slicer_x"], g["slicer_y"], "BinarySlicer")
    for m in (2, 4):
        whole_and_cut(lambda: dsp.DifferentialDecoder(m, int(g[f"diff{m}_init"])), g[f"diff{m}_x"], g[f"diff{m}_y"],
                      f"DifferentialDecoder {m}")


# ----------------------------------------------------------------------- MM
def mm_checks(make, t, what):
    """`make(omega, omega_gain, mu_gain, rel, P, T)` -> a block with process / reset / set_omega, against
    every MM fixture of type `t` ("f" or "c")."""
    g = load("mm")
    for name, kind in (("a", "psk"), ("b", "noise"), ("c", "noise")):
        x, want = g[f"x_{kind}_{t}"], g[f"mm_{name}_{t}_y"]
        p = tuple(g[f"mm_{name}_{t}_params"])
        assert len(want) > N / p[0] * 0.98 - 2
        y = make(*p, 128, 8).process(x)
        assert len(y) == len(want), f"{what} {name}: {len(y)} outputs, the reference {len(want)}"
        assert same(y, want), f"{what} {name}"
        calls = in_calls(make(*p, 128, 8), x)
        assert [len(c) for c in calls] == list(g[f"mm_{name}_{t}_cut_counts"]), f"{what} {name}: per-call counts"
        assert same(np.concatenate(calls), want), f"{what} {name}: in calls"
    x = g[f"x_psk_{t}"]
    assert same(make(*MM_BASE, 64, 8).process(x), g[f"mm_interp64_{t}_y"]), f"{what}: interpolator (64, 8)"
    # 3001 samples, reset() (the 7 history samples stay), 2999 samples, setOmega(5000 / 1187.5), 6000 samples
    m = make(*MM_BASE, 128, 8)
    out = [m.process(x[:3001])]
    m.reset()
    out.append(m.process(x[3001:6000]))
    m.set_omega(float(g["mm_ops_omega2"]))
    out.append(m.process(x[6000:]))
    assert float(g["mm_ops_omega2"]) == OM2
    assert [len(c) for c in out] == list(g[f"mm_ops_{t}_counts"]), f"{what}: counts around reset / setOmega"
    assert same(np.concatenate(out), g[f"mm_ops_{t}_y"]), f"{what}: outputs around reset / setOmega"


class ClampCountingMM(R.RefMM):
    hits = None

    def clamp_freq(self):
        before = self.freq
        super().clamp_freq()
        if self.hits is not None and self.freq != before:
            self.hits.add("max" if self.freq < before else "min")


@pytest.mark.parametrize("t", ["f", "c"])
def test_mm_restatement_is_the_reference(t):
    mm_checks(lambda om, og, mg, rel, P, T: R.RefMM(om, og, mg, rel, P, T, cplx=t == "c"), t, "RefMM")
    # case c is there for the frequency clamp (before the phase update, phase_control_loop.h:60-64): it engages
    g = load("mm")
    m = ClampCountingMM(*g[f"mm_c_{t}_params"], cplx=t == "c")
    m.hits = set()
    m.process(g[f"x_noise_{t}"])
    assert m.hits == {"min", "max"}, f"omega reached {sorted(m.hits)} only"


@gpu
@pytest.mark.parametrize("t", ["f", "c"])
def test_mm_device_is_the_reference(t):
    mm_checks(lambda om, og, mg, rel, P, T: dsp.MM(om, og, mg, rel, P, T, complex_data=t == "c"), t, "MM")


# ------------------------------------------------------------------- Costas
def costas_fixture(case):
    g = load("costas_a" if case in ("order2", "order4") else "costas_b")
    return g[f"{case}_x"], g[f"{case}_y"]


@pytest.fixture(scope="module")
def costas_refs():
    return {case: R.costas_ref_and_S(case) for case in R.COSTAS_CASES}


def costas_bar(r):
    return 16 * max(r["S"], 4 * float(EPS32) * float(np.abs(r["ref"]).max()))


@pytest.mark.parametrize("case", sorted(R.COSTAS_CASES))
def test_costas_restatement_within_the_loops_own_sensitivity(case, costas_refs):
    x, want = costas_fixture(case)
    r = costas_refs[case]
    assert same(x, r["x"]), "the fixture's input is not the suite's"
    d, bar = gap(r["ref"], want), costas_bar(r)
    print(f"costas {case}: S {r['S']:.3e}, restatement (fp64 trig) to reference {d:.3e}, bar {bar:.3e}")
    write_report("ref_pin", {"case": f"costas_{case}", "S": r["S"], "bar": bar, "restatement_gap": d})
    assert d <= bar


@gpu
@pytest.mark.parametrize("case", sorted(R.COSTAS_CASES))
def test_costas_device_within_the_loops_own_sensitivity(case, costas_refs):
    x, want = costas_fixture(case)
    c, kw = R.COSTAS_CASES[case], R.COSTAS_CASES[case]["kw"]
    make = lambda: dsp.Costas(c["order"], c["bandwidth"], kw.get("init_phase", 0.0), kw.get("init_freq", 0.0),
                              kw.get("min_freq", -float(R.FL_M_PI)), kw.get("max_freq", float(R.FL_M_PI)))
    y = make().process(x)
    z = np.concatenate(in_calls(make(), x))
    assert same(y, z), "the stream in calls differs from one call"
    d, bar = gap(y, want), costas_bar(costas_refs[case])
    print(f"costas {case}: device to reference {d:.3e}, bar {bar:.3e}")
    write_report("ref_pin", {"case": f"costas_{case}", "bar": bar, "device_gap": d})
    assert d <= bar


# ------------------------------------------------- noise blanker, squelch, FMIF
def test_noise_blanker_restatement_is_the_reference():
    g = load("ifnr")
    for k in (0, 1):
        rate, level = g[f"nb{k}_params"]
        assert np.any(g[f"nb{k}_y"] != g["nb_x"]), "the input never tripped the blanker"
        whole_and_cut(lambda: R.NoiseBlankerRef(rate, level), g["nb_x"], g[f"nb{k}_y"], f"NoiseBlankerRef {k}")


@gpu
def test_noise_blanker_device_is_the_reference():
    g = load("ifnr")
    for k in (0, 1):
        rate, level = g[f"nb{k}_params"]
        whole_and_cut(lambda: dsp.NoiseBlanker(float(rate), float(level)), g["nb_x"], g[f"nb{k}_y"], f"NoiseBlanker {k}")


def squelch_case():
    g = load("ifnr")
    x, is_open = g["squelch_x"], g["squelch_open"]
    assert x.shape == (len(R.SQ_SEQUENCE), R.SQ_N) and same(x, np.stack(R.squelch_blocks()))
    # what the sequence is meant to exercise (test_ifnr.py test_squelch_sequence), by the reference itself
    want = [True, False] + [False] * 10 + [True, True, False] + [False] * 3 + [False] + [False] * 9 + [True, True]
    assert list(is_open) == want
    return float(g["squelch_level"]), x, is_open


def test_squelch_restatement_is_the_reference():
    level, x, is_open = squelch_case()
    r = R.SquelchRef(level)
    for j, b in enumerate(x):
        y = r.process(b)
        assert (not r.muted) == is_open[j], f"block {j}: restated {'open' if not r.muted else 'closed'}"
        assert same(y, b if is_open[j] else np.zeros_like(b)), j


@gpu
def test_squelch_device_is_the_reference():
    level, x, is_open = squelch_case()
    s = dsp.Squelch(level)
    for j, b in enumerate(x):
        y = s.process(b)
        assert (not s.is_muted()) == is_open[j], f"block {j}: device {'closed' if s.is_muted() else 'open'}"
        assert same(y, b if is_open[j] else np.zeros_like(b)), j


@pytest.mark.parametrize("kind", ["fm", "uniform"])
@pytest.mark.parametrize("B", [3, 16, 31])
def test_fmif_bar_passes_the_reference(B, kind):
    g = load("ifnr")
    x, y = g[f"fmif_x_{kind}"], g[f"fmif_y_{kind}_{B}"]
    assert len(x) == 3000 and same(x, R.fmif_inputs(kind, n=3000))
    share = R.fmif_check(y, x, B, f"reference B={B} {kind}")
    assert share <= 0.01, f"undecidable share {share:.4%} > 1 %"


# --------------------------------------------- AGC, DC blocker, de-emphasis
def loop_cases(lib, t):
    """(name, make, x, want, want_cut) of the serial loops in library `lib` (oracle or dsp), t in "f", "c"."""
    a, b = load("loops_a"), load("loops_b")
    cd = t == "c"
    args = tuple(float(v) for v in a["agc_params"])
    if lib is oracle:
        agc, dcb = (lambda: oracle.AGC(cd, *args)), (lambda: oracle.DCBlocker(float(b["dcb_rate"]), cd))
    else:
        agc, dcb = (lambda: dsp.AGC(*args, complex_data=cd)), (lambda: dsp.DCBlocker(float(b["dcb_rate"]), cd))
    yield "AGC", agc, a[f"x_{t}"], a[f"agc_{t}_y"], a[f"agc_{t}_y_cut"]
    yield "DCBlocker", dcb, b[f"x_{t}"], b[f"dcb_{t}_y"], None
    tau, fs = (float(v) for v in b["deemp_params"])
    if cd:                                                      # stereo_t pairs: (l, r) = (re, im)
        yield ("Deemphasis stereo", lambda: lib.Deemphasis(tau, fs, True), b["x_c"].view(lib.STEREO),
               b["deemp_s_y"].view(lib.STEREO), None)
    else:
        yield "Deemphasis", (lambda: lib.Deemphasis(tau, fs, False)), b["x_f"], b["deemp_f_y"], None


def run_loop_cases(lib, t):
    for name, make, x, want, want_cut in loop_cases(lib, t):
        if name == "AGC":
            assert not same(want, want_cut), "the cuts never end inside a clip look-ahead: they show nothing"
        whole_and_cut(make, x, want, f"{lib.__name__} {name} {t}", want_cut)


@pytest.mark.parametrize("t", ["f", "c"])
def test_oracle_loops_are_the_reference(t):
    run_loop_cases(oracle, t)


@gpu
@pytest.mark.parametrize("t", ["f", "c"])
def test_device_loops_are_the_reference(t):
    run_loop_cases(dsp, t)


# -------------------------------------------------------------- design code
def test_host_design_code_is_the_reference():
    g = np.load(os.path.join(GOLDEN, "ref_blocks_design.npz"))
    seen = {"rrc": 0, "mmbank": 0, "fmifwin": 0}
    for k in g.files:
        kind = k.split("_")[0]
        if k.endswith("_args"):
            continue
        if kind == "rrc":
            count, beta, Ts = g[k + "_args"]
            got = dsp.root_raised_cosine(int(count), float(beta), float(Ts))
        elif kind == "mmbank":
            got = dsp.mm_interp_bank(*map(int, k.split("_")[1:]))
        else:
            got = dsp.fmif_window(int(k.split("_")[1]))
        assert same(got, g[k]), k
        seen[kind] += 1
    assert seen == {"rrc": 4, "mmbank": 3, "fmifwin": 6}


# ------------------------------------------------------------------- chains
CHAINS = {
    # name: (fixture file, settling prefix in symbols, the hard decision, the distance to its boundary)
    "psk2": ("chains_a", 1000, R.quadrant, lambda y: np.minimum(np.abs(y.real), np.abs(y.imag))),
    "psk4": ("chains_a", 1000, R.quadrant, lambda y: np.minimum(np.abs(y.real), np.abs(y.imag))),
    "gfsk": ("chains_a", 1000, R.ref_slicer, np.abs),
    "rds0": ("chains_b", 600, R.ref_slicer, np.abs),
    "rds1": ("chains_b", 600, R.ref_slicer, np.abs),
}


def chain_case(name):
    fname, lo, decide, margin = CHAINS[name]
    g = load(fname)
    y, z = g[f"{name}_y"], g[f"{name}_y_sum4"]
    s_chain = gap(y[lo:], z[lo:]) if len(y) == len(z) else float("nan")
    bar = 16 * max(s_chain, 4 * float(EPS32) * float(np.abs(y[lo:]).max()))
    return g, lo, decide, margin, y, z, s_chain, bar


def restated_chain(name, g, lanes, trig):
    """The chain restated block by block (tests/_restated.py), its FIR dot products summed in `lanes`
    partial sums and its Costas phasor from `trig`. Returns (soft outputs, phase * P of every output)."""
    x = g[f"{name}_x"]
    if name.startswith("psk"):
        order, symrate, fs, ntaps, beta, agc_rate, bw, og, mg, rel = g[f"{name}_params"]
        f = R.ref_fir32(x, dsp.root_raised_cosine(int(ntaps), beta, fs / symrate), lanes)     # psk.h:31-32, :139
        ar, ai, _ = R.ref_fast_agc(*parts(f), 1.0, 10e6, agc_rate, f32(1.0))                   # :33, :140
        cr, ci = R.ref_costas(ar, ai, int(order), bw, trig=trig)                               # :34, :141
        mm, z = R.RefMM(fs / symrate, og, mg, rel, cplx=True), cplx(cr, ci)                    # :35, :142
    elif name == "gfsk":
        symrate, fs, dev, ntaps, beta, og, mg, rel = g["gfsk_params"]
        q = oracle.Quadrature(2 * np.pi * dev / fs).process(x)                                 # gfsk.h:31, :132
        z = R.ref_fir32(q, dsp.root_raised_cosine(int(ntaps), beta, fs / symrate), lanes)     # :32-33, :133
        mm = R.RefMM(fs / symrate, og, mg, rel)                                                # :34, :134
    else:
        w = R.W_RDS
        yr, yi, _ = R.ref_fast_agc(*parts(x), 1.0, 1e6, 0.1, f32(1.0))                         # wfm.h:57
        yr, yi = R.ref_costas(yr, yi, 2, f32(0.005), trig=trig)                                # :58
        f = R.ref_fir32(cplx(yr, yi), dsp.band_pass(0, 2375, 100, 5000, complex_taps=True), lanes)   # :60-61
        cr, _ = R.ref_costas(*parts(f), 2, 0.01, 0.0, w, w - (w * 0.1), w + (w * 0.1), trig=trig)   # :63-64
        mm, z = R.RefMM(5000.0 / (2375.0 / 2.0), 1e-6, 0.01, 0.01), cr[0]                       # :66-67
    mm.trace = []
    return mm.process(z), np.array(mm.trace, f32)


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_chain_inputs_meet_the_preconditions(name):
    g, lo, decide, margin, y, z, s_chain, bar = chain_case(name)
    x = g[f"{name}_x"]
    # the input is the known-answer signal and the reference alone recovers what was sent
    if name.startswith("psk"):
        order = int(name[3])
        sig, q = R.shaped_psk(int(g[f"{name}_signal"][0]), order, amp=0.05)
        assert tuple(g[f"{name}_params"]) == (order,) + R.PSK_ARGS
        sym = R.quadrant(y) if order == 4 else (y.real > 0).astype(int)
        e, lag = R.errors_at_best_lag(np.diff(sym) % order, np.diff(q) % order, range(40), 1000, 2800)
    elif name == "gfsk":
        sig, b = R.gfsk_signal(int(g["gfsk_signal"][0]))
        assert tuple(g["gfsk_params"]) == R.GFSK_ARGS
        e, lag = R.errors_at_best_lag(R.ref_slicer(y), b.astype(np.uint8), range(40), 1000, 2800)
    else:
        f0, snr_db, seed = g[f"{name}_signal"]
        sig, b = R.rds_signal(f0, snr_db, int(seed))
        bits = g[f"{name}_bits"]
        assert same(bits, R.ref_diff(R.ref_slicer(y), 2)) and same(g[f"{name}_bits_sum4"], R.ref_diff(R.ref_slicer(z), 2))
        e, lag = R.errors_at_best_lag(bits, b, range(80), 600, min(len(b), len(bits)) - 80)
    assert same(x, sig), "the fixture's input is not the suite's known-answer signal"
    assert e == 0, f"the reference alone does not recover what was sent: {e} errors at lag {lag}"
    # both builds: equal counts, identical hard decisions; no symbol within the bar of a boundary
    assert len(y) == len(z), f"the two reference builds give {len(y)} and {len(z)} outputs"
    assert sum(g[f"{name}_cut_counts"]) == len(y)
    assert np.array_equal(decide(y[lo:]), decide(z[lo:])), "the two reference builds decide differently"
    m = float(margin(y[lo:]).min())
    print(f"{name}: {len(y)} outputs, S_chain {s_chain:.3e}, bar {bar:.3e}, smallest distance to a decision boundary {m:.3e}")
    write_report("ref_pin", {"case": f"chain_{name}", "outputs": len(y), "S_chain": s_chain, "bar": bar, "min_margin": m})
    assert m > bar, f"a symbol lies {m:.3e} from a decision boundary, inside the bar {bar:.3e}"
    # the restated chain is the reference's to within the bar, and every symbol's interpolator branch is decided
    r1, u1 = restated_chain(name, g, 1, R.trig64)
    assert len(r1) == len(y)
    d = gap(r1[lo:], y[lo:])
    s_u = 0.0
    for lanes, trig in ((1, R.trig32), (4, R.trig32), (4, R.trig64)):
        r, u = restated_chain(name, g, lanes, trig)
        assert len(r) == len(y), f"the chain restated with {lanes}-lane sums gives {len(r)} outputs"
        s_u = max(s_u, gap(u1[lo:], u[lo:]))
    u_bar = 2 * max(s_u, 4 * float(EPS32) * float(u1.max()))
    m_u = float(np.abs(u1[lo:] - np.round(u1[lo:])).min())
    print(f"{name}: restated chain to reference {d:.3e}; phase x P: S_u {s_u:.3e}, bar {u_bar:.3e}, "
          f"smallest distance to a branch boundary {m_u:.3e}")
    write_report("ref_pin", {"case": f"chain_{name}", "restatement_gap": d, "S_u": s_u, "u_bar": u_bar, "min_branch_margin": m_u})
    assert d <= bar
    assert m_u > u_bar, f"a symbol's phase x P lies {m_u:.3e} from an integer, inside {u_bar:.3e}"


def device_chain(name, g):
    if name.startswith("psk"):
        return lambda: dsp.PSK(*g[f"{name}_params"])
    if name == "gfsk":
        return lambda: dsp.GFSK(*g["gfsk_params"])
    return dsp.RDSBits


@gpu
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_chain_device_against_the_reference(name):
    g, lo, decide, margin, want, _, s_chain, bar = chain_case(name)
    x = g[f"{name}_x"]
    make = device_chain(name, g)
    blk = make()
    y = blk.process(x)
    if name.startswith("rds"):
        bits, y = y, blk.symbols()
        assert len(bits) == len(y)
    assert len(y) == len(want), f"{len(y)} outputs, the reference {len(want)}"
    calls = in_calls(make(), x)
    assert [len(c) for c in calls] == list(g[f"{name}_cut_counts"]), "per-call counts"
    assert same(np.concatenate(calls), bits if name.startswith("rds") else y), "the stream in calls differs from one call"
    d = gap(y[lo:], want[lo:])
    print(f"{name}: S_chain {s_chain:.3e}, device to reference {d:.3e}, bar {bar:.3e}")
    write_report("ref_pin", {"case": f"chain_{name}", "bar": bar, "device_gap": d})
    assert np.array_equal(decide(y[lo:]), decide(want[lo:])), "hard decisions differ from the reference's"
    if name.startswith("rds"):
        assert same(bits[lo + 1:], g[f"{name}_bits"][lo + 1:]), "bits differ from the reference's"
    assert d <= bar


# --------------------------------------------------------------- live probe
@pytest.mark.skipif(not have_reference(), reason="reference tree not mounted (GPU box): the committed fixtures cover it")
def test_live_reference_probe_reproduces_the_fixtures():
    assert_live_probe_reproduces("ref_blocks_", "blocks_fixtures")
