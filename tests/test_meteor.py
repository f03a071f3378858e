"""The Meteor (LRPT) demodulator and the carrier loops on the device (libsdrgpu, HIP): PLL, CarrierPLL, MeteorCostas
and Meteor against the numpy float32 restatements of tests/_meteor.py (one scalar operation per reference operation;
tests/test_meteor_ref.py holds them to the reference's own code).

Bars:
* MeteorCostas without broken modulation -- bit-identical to dsp.Costas(4, ...): its error is Costas<4>'s to the letter.
* MeteorCostas with broken modulation, PLL, CarrierPLL -- cosf / sinf / atan2f are the device libm's: the project's
  sensitivity bar (test_symsync.py). S = the largest gap between the fp32-trig and fp64-trig restatements over 8 seeds;
  the device must be within 16 max(S, 4 eps32 max|y|) of the fp64-trig run. The bar never comes from device numbers.
  A bar above 1 % of the constellation radius would show nothing, and neither would a loop that does not lock: each
  case's signal and bandwidth are chosen so that the restatement locks (the residual rotation of its tail) and the
  bar stays under that, both asserted on the restatement before the device is looked at.
* A run in CUTS is bit-identical to one call on a fresh handle; after reset a block is bit-identical to a fresh one;
  zero input gives exact +-0 from the two loops that derotate their input.
* set_broken_modulation at a call boundary -- within the bar of the restatement switched at the same sample; it does
  not reset the loop.
* Meteor -- bit-identical to the RRC FIR -> dsp.FastAGC -> dsp.MeteorCostas -> the stagger in numpy (pure data
  movement, lastI carried across calls) -> dsp.MM, for the four (broken, oqpsk) combinations, whole and in cuts;
  set_oqpsk off and on keeps the stale lastI; reset keeps lastI and MM's history. The FIR part is the FIR that sums
  as the reference's VOLK generic kernel does (ascending taps, fp32, unfused), reached as a one-stream dsp.BankFIR:
  Meteor's RRC runs that kernel, so that a BankMeteor column is the single-stream chain bit for bit and the chain
  differs from the reference by its libm alone. dsp.FIR picks its kernel and summation order by shape and contracts
  (it is held to a tolerance), so it cannot be bit-identical to the bank FIR and stand in here as well.
* Known answers -- the fp64-trig restatement alone must recover the transmitted symbols with 0 errors at the best
  lag, then the device must, with a symbol count within 1 of the restatement's. QPSK and OQPSK: the differential
  quadrant; broken modulation: the nearest PHASE constant (its four phases are unevenly spaced: no ambiguity).
  OQPSK: the reference delays the Q arm by one more sample (meteor_demod.h:157-161) where the signal's Q arm is one
  sample late already, so a symbol pairs I of symbol k with Q of symbol k - 1 or, with the loop locked a quarter turn
  on, I and Q of one symbol: both pairings are scored and the better one counts.
Recorded through write_report: meteor_parity."""
import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import dsp
from _util import write_report
from _restated import N, CUTS, FL_M_PI, bits, same, errors_at_best_lag, quadrant
import _meteor as M

pytestmark = pytest.mark.gpu
PI = float(FL_M_PI)
RADIUS = 1.0                                                     # unit-rms inputs; the AGC's set point


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"


def in_calls(block, x):
    out, i = [], 0
    for c in CUTS:
        out.append(block.process(x[i:i + c]))
        i += c
    assert i == len(x) == N
    return np.concatenate(out)


def whole_and_cut(make, x, what):
    y = make().process(x)
    z = in_calls(make(), x)
    assert same(y, z), f"{what}: the stream in calls differs from one call"
    return y


# ------------------------------------------------ MeteorCostas is Costas<4>
def test_meteor_costas_without_broken_modulation_is_costas4_bit_for_bit():
    x = M.loop_ref_and_S("meteor_costas_plain")["x"]
    y = whole_and_cut(lambda: dsp.MeteorCostas(M.COSTAS_BW, False), x, "meteor_costas plain")
    assert same(y, dsp.Costas(4, M.COSTAS_BW).process(x))
    # other limits and initial state, through the setters too
    a, b = dsp.MeteorCostas(0.02, False, 0.3, 0.01, -0.5, 0.5), dsp.Costas(4, 0.005, 0.3, 0.01, -1.0, 1.0)
    b.set_bandwidth(0.02)
    b.set_freq_limits(-0.5, 0.5)
    assert same(a.process(x[:3000]), b.process(x[:3000]))


# ----------------------------------------------------- the loops' own bar
def locked_pll(r):
    """The VCO's phasor follows the clean carrier: their mean product over the tail has modulus ~1 (not a spinning copy)."""
    clean = np.exp(1j * (0.05 * np.arange(N) + 0.4))
    return abs(np.mean(r["ref"][6000:].astype(np.complex128) * np.conj(clean[6000:]))) > 0.99


def locked_carrier_pll(r):
    """The derotated carrier sits on the real axis at its amplitude in both halves of the tail."""
    t = r["ref"][6000:].astype(np.complex128)
    return all(abs(np.angle(np.mean(h))) < 0.01 and abs(np.mean(h).real - 0.5) < 0.01 for h in (t[:3000], t[3000:]))


def locked_broken(r):
    """The residual rotation of the strong samples against their nearest PHASE constant, in both halves of the tail."""
    z = r["ref"].astype(np.complex128)
    res = []
    for a, b in ((6000, 9000), (9000, 12000)):
        zz = z[a:b][np.abs(z[a:b]) > 0.8]
        res.append(abs(np.angle(np.mean(zz * np.exp(-1j * M.PHASES.astype(np.float64)[M.nearest_phase(zz)])))))
    return max(res) < 0.01


LOOPS = {
    "pll": (lambda: dsp.PLL(M.LOOP_BW), locked_pll, False),
    "carrier_pll": (lambda: dsp.CarrierPLL(M.LOOP_BW), locked_carrier_pll, True),
    "meteor_costas_broken": (lambda: dsp.MeteorCostas(M.COSTAS_BW, True), locked_broken, True),
}


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_loop_within_its_own_sensitivity(name):
    make, locked, derotates = LOOPS[name]
    r = M.loop_ref_and_S(name)
    assert locked(r), "restatement did not lock"
    assert r["bar"] < 0.01 * RADIUS, "a bar above 1 % of the radius shows nothing"
    y = whole_and_cut(make, r["x"], name)
    dev = M.gap(y, r["ref"])
    print(f"{name}: S {r['S']:.3e}, device deviation {dev:.3e}, bar {r['bar']:.3e}")
    write_report("meteor_parity", {"case": name, "S": r["S"], "bar": r["bar"], "device_to_restatement": dev})
    assert dev <= r["bar"]
    # reset -> the initial phase and frequency
    m = make()
    m.process(r["x"][:2500])
    m.reset()
    assert same(m.process(r["x"][:2000]), y[:2000])
    if derotates:
        z = whole_and_cut(make, np.zeros(N, np.complex64), f"{name} zeros")
        assert z.shape == (N,) and not np.any(bits(z) & np.uint64(0x7FFFFFFF7FFFFFFF))   # +-0 only


def test_pll_setters():
    x = M.loop_ref_and_S("pll")["x"]
    for cls in (dsp.PLL, dsp.CarrierPLL):
        a, b = cls(M.LOOP_BW), cls(0.05, 0.0, 0.0, -0.5, 0.5)
        b.set_bandwidth(M.LOOP_BW)
        b.set_freq_limits(-PI, PI)
        assert same(a.process(x[:3000]), b.process(x[:3000]))
        # setFrequencyLimits clamps the running frequency (0.05 rad/sample here) at the next call
        a.set_freq_limits(-0.01, 0.01)
        c = cls(M.LOOP_BW, 0.0, 0.0, -0.01, 0.01)
        assert not same(a.process(x[3000:3500]), c.process(x[3000:3500]))   # (a keeps its phase)


def test_set_broken_modulation_mid_stream():
    r = M.loop_ref_and_S("meteor_costas_switch")
    assert locked_broken(r) and r["bar"] < 0.01 * RADIUS
    x, at = r["x"], M.SWITCH_AT
    m = dsp.MeteorCostas(M.COSTAS_BW, False)
    m.set_broken_modulation(True)
    m.set_broken_modulation(False)                               # only the value at the call counts
    y = [m.process(x[:at])]
    assert same(y[0], dsp.Costas(4, M.COSTAS_BW).process(x[:at]))
    m.set_broken_modulation(True)                                # from the next call
    y.append(m.process(x[at:]))
    y = np.concatenate(y)
    dev = M.gap(y, r["ref"])
    print(f"meteor_costas switch: S {r['S']:.3e}, device deviation {dev:.3e}, bar {r['bar']:.3e}")
    write_report("meteor_parity", {"case": "meteor_costas_switch", "S": r["S"], "bar": r["bar"], "device_to_restatement": dev})
    assert dev <= r["bar"]
    fresh = dsp.MeteorCostas(M.COSTAS_BW, True).process(x[at:])
    assert M.gap(fresh[:50], y[at:at + 50]) > 100 * r["bar"], "the loop state does not matter here: the check would show nothing"


# ------------------------------------------------------- Meteor is its parts
class OrderedFIR:
    """filter::FIR<complex_t, float> summed in ascending tap order, fp32, unfused, on one stream: a one-stream BankFIR."""

    def __init__(self, taps):
        self.bank = dsp.BankFIR(1, taps)

    def process(self, x):
        return np.ascontiguousarray(self.bank.process(np.ascontiguousarray(x)[:, None])[:, 0])

    def reset(self):
        self.bank.reset()


class Parts:
    """demod::Meteor's stages as single blocks, the stagger (meteor_demod.h:155-161) on the host between them."""

    def __init__(self, broken, oqpsk):
        a = M.meteor_args(broken, oqpsk)
        self.blocks = [OrderedFIR(dsp.root_raised_cosine(a[2], a[3], a[1] / a[0])), dsp.FastAGC(1.0, 10e6, a[4], complex_data=True),
                       dsp.MeteorCostas(a[5], broken), dsp.MM(a[1] / a[0], a[8], a[9], a[10], complex_data=True)]
        self.oqpsk, self.last_i = oqpsk, np.float32(0)

    def process(self, x):
        for b in self.blocks[:3]:
            x = b.process(x)
        if self.oqpsk and len(x):
            im = np.concatenate([[self.last_i], x.imag]).astype(np.float32)
            self.last_i = im[-1]
            x = (x.real + 1j * im[:-1]).astype(np.complex64)
        return self.blocks[3].process(x)

    def reset(self):                                             # the four blocks, not lastI
        for b in self.blocks:
            b.reset()


@pytest.mark.parametrize("broken,oqpsk", [(False, False), (True, False), (False, True), (True, True)])
def test_meteor_is_its_parts(broken, oqpsk):
    x = M.meteor_ref_and_S("broken" if broken else ("oqpsk" if oqpsk else "qpsk"))["x"]
    y = whole_and_cut(lambda: dsp.Meteor(*M.meteor_args(broken, oqpsk)), x, f"meteor {broken} {oqpsk}")
    z = Parts(broken, oqpsk).process(x)
    assert len(y) == len(z) and abs(len(y) - M.NSYM) <= 2 and same(y, z)
    assert same(in_calls(Parts(broken, oqpsk), x), z)
    if oqpsk:
        plain = dsp.Meteor(*M.meteor_args(broken, False)).process(x)
        assert not same(plain[:len(y)], y[:len(plain)]), "the stagger does not matter here: the check would show nothing"


def test_meteor_set_oqpsk_keeps_the_stale_carry_and_reset_keeps_it_too():
    x = M.meteor_ref_and_S("ops")["x"]
    m, p = dsp.Meteor(*M.meteor_args(*M.OPS_START)), Parts(*M.OPS_START)
    at = 0
    for op in M.METEOR_OPS:
        if op == "r":
            m.reset()
            p.reset()
        elif isinstance(op, str) and op[0] == "q":
            m.set_oqpsk(op[1] == "1")
            p.oqpsk = op[1] == "1"
        elif isinstance(op, str):
            m.set_broken_modulation(op[1] == "1")
            p.blocks[2].set_broken_modulation(op[1] == "1")
        else:
            a, b = m.process(x[at:at + op]), p.process(x[at:at + op])
            assert same(a, b), f"the {op} samples from {at}"
            at += op
    assert at == N and p.last_i != 0
    # after reset: the loops as a fresh handle's, but the carry and MM's 7 history samples stay
    m.set_broken_modulation(False)
    p.blocks[2].set_broken_modulation(False)
    m.reset()
    p.reset()
    a, fresh = m.process(x[:500]), dsp.Meteor(*M.meteor_args(*M.OPS_START)).process(x[:500])
    assert same(a, p.process(x[:500])) and not same(a[:4], fresh[:4])


def test_mm_setters_reach_the_meteor_chain():
    x = M.meteor_ref_and_S("qpsk")["x"][:4000]
    m = dsp.Meteor(*M.meteor_args(False, False))
    m.set_gains(1e-5, 0.02)
    m.set_omega_rel_limit(0.02)
    m.set_costas_bandwidth(0.01)
    a = M.meteor_args(False, False)
    ps = [OrderedFIR(dsp.root_raised_cosine(33, 0.6, a[1] / a[0])), dsp.FastAGC(1.0, 10e6, 0.1, complex_data=True),
          dsp.MeteorCostas(0.01, False), dsp.MM(a[1] / a[0], 1e-5, 0.02, 0.02, complex_data=True)]
    y = x
    for b in ps:
        y = b.process(y)
    assert same(m.process(x), y)
    with pytest.raises(sdrpp_amd.SdrGpuError):
        m.set_omega(1.0)                                         # an output would consume no input


# ------------------------------------------------------------ known answers
def symbol_errors(name, y, q):
    lo, hi = 1500, 5000
    if name == "broken":
        return errors_at_best_lag(M.nearest_phase(y), q, range(40), lo, hi)
    if name == "qpsk":
        return errors_at_best_lag(np.diff(quadrant(y)) % 4, np.diff(q) % 4, range(40), lo, hi)
    i, qq = np.cos(np.pi / 4 + q * np.pi / 2), np.sin(np.pi / 4 + q * np.pi / 2)
    pairings = [i[1:] + 1j * qq[1:], i[1:] + 1j * qq[:-1]]       # I and Q of one symbol; I of symbol k with Q of symbol k - 1
    return min(errors_at_best_lag(np.diff(quadrant(y)) % 4, np.diff(quadrant(z)) % 4, range(40), lo, hi) for z in pairings)


@pytest.mark.parametrize("name", ["qpsk", "broken", "oqpsk"])
def test_known_answer(name):
    r = M.meteor_ref_and_S(name)
    q = M.lrpt_signal(M.METEOR_SEEDS[name][0], name)[1]
    e, lag = symbol_errors(name, r["ref"], q)
    print(f"{name}: restatement {e} errors at lag {lag}, {len(r['ref'])} symbols")
    assert e == 0, "the restatement alone does not recover the symbols"
    y = dsp.Meteor(*M.meteor_args(*M.METEOR_CASES[name])).process(r["x"])
    e, lag = symbol_errors(name, y, q)
    print(f"{name}: device {e} errors at lag {lag}, {len(y)} symbols")
    write_report("meteor_parity", {"case": f"known_answer_{name}", "device_errors": e, "symbols": len(y), "restated_symbols": len(r["ref"])})
    assert e == 0 and abs(len(y) - len(r["ref"])) <= 1
