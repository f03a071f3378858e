"""The Meteor demodulator and the carrier loops against the REFERENCE's own code: tests/golden/ref_meteor_*.npz hold
what loop::PLL, loop::CarrierTrackingPLL, loop::MeteorCostas and demod::Meteor compute, run from the reference's headers
by oracle/ref_blocks.cpp's pll, cpll, mcostas and meteor modes (tools/gen_ref_fixtures.py meteor_fixtures).

CPU: every restatement of tests/_meteor.py reproduces the fixtures -- whole calls and cuts (the generator asserts that
the reference gives the same outputs either way and keeps them once; the demodulator's per-call counts are kept for
the cut feed), reset, setBrokenModulation and setOQPSK mid-stream. Where the reference tree is present, a fresh probe
build must reproduce the committed files byte for byte.
gpu: the device blocks are held to the same fixtures and the same bars.

Bars. Every loop here goes through cosf / sinf or atan2f, which no two libms round alike: the project's sensitivity bar
(test_symsync.py): S = the largest gap between the fp32-trig and fp64-trig restatements over the case's 8 seeds, bar =
16 max(S, 4 eps32 max|y|). No bar comes from device numbers. MeteorCostas without broken modulation is bit-identical to
the restated Costas<4> (ref_costas) as well. The demodulator's counts are exact: 0 differing counts allowed. Its
streams (tests/_meteor.py METEOR_SEEDS, which says why) are those on which both restatements agree on every count and
every decision of MM, the fixture's stream being the one whose decisions stay farthest from their boundaries (at least
MM_MARGIN); that precondition, and that the bar stays under 1 % of the constellation radius, are asserted on the
restatements alone. Recorded through write_report: meteor_parity."""
import os

import numpy as np
import pytest

import sdrpp_amd
from sdrpp_amd import dsp
from _util import GOLDEN, assert_live_probe_reproduces, have_reference, write_report
from _restated import N, CUTS, FL_M_PI, same, parts, ref_costas
import _meteor as M

RADIUS = 1.0                                                     # the AGC's set point (meteor_demod.h:33)
PI = float(FL_M_PI)
gpu = pytest.mark.gpu


def load(name):
    return np.load(os.path.join(GOLDEN, f"ref_meteor_{name}.npz"))


def parse_ops(s):
    return [int(t) if t.lstrip("-").isdigit() else t for t in str(s).split(",")]


def c64(pair, k=0):
    return (pair[0][k] + 1j * pair[1][k]).astype(np.complex64)


def held(what, y, ref, bar, S, kind):
    d = M.gap(y, ref)
    print(f"{what}: S {S:.3e}, {kind} gap {d:.3e}, bar {bar:.3e}")
    write_report("meteor_parity", {"case": what, "S": S, "bar": bar, f"{kind}_gap": d})
    assert len(y) == len(ref) and d <= bar, what


# ------------------------------------------------------------------- CPU: the loops
LOOPS = {"pll": ("loops", "pll_y", "pll"), "carrier_pll": ("loops", "cpll_y", "carrier_pll"),
         "meteor_costas_plain": ("costas", "qpsk_y", "meteor_costas_plain"),
         "meteor_costas_broken": ("costas", "broken_y", "meteor_costas_broken")}


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_loop_restatements_reproduce_the_reference(name):
    fname, key, case = LOOPS[name]
    g, r = load(fname), M.loop_ref_and_S(case)
    x = g["x"] if fname == "loops" else g["x_qpsk" if name.endswith("plain") else "x_broken"]
    assert same(x, r["x"]), "the fixture's input is not the case's seed 0"
    assert r["bar"] < 0.01 * RADIUS, "a bar above 1 % of the radius shows nothing"
    for kind in ("ref", "ref32"):
        held(f"{name} {kind}", r[kind], g[key], r["bar"], r["S"], "restatement")


def test_meteor_costas_without_broken_modulation_is_costas4():
    x = M.loop_ref_and_S("meteor_costas_plain")["x"]
    xr, xi = parts(x)
    for trig, cs in ((M.trig32, M.trig32.cs), (M.trig64, M.trig64.cs)):
        a = M.ref_meteor_costas(xr, xi, M.COSTAS_BW, False, trig)
        b = ref_costas(xr, xi, 4, M.COSTAS_BW, trig=cs)
        assert same(a[0], b[0]) and same(a[1], b[1])


@pytest.mark.parametrize("name", ["pll", "carrier_pll"])
def test_loop_restatements_reset(name):
    g, r = load("loops"), M.loop_ref_and_S(name)
    assert parse_ops(g["ops"]) == M.LOOP_OPS
    xr, xi = parts(r["x"])
    pcl, out, at = M.Pcl(1, M.LOOP_BW), [], 0
    for op in M.LOOP_OPS:
        if op == "r":
            pcl.reset()
            continue
        out.append(c64(M.pll_run(pcl, xr[:, at:at + op], xi[:, at:at + op], M.trig64, name == "carrier_pll")))
        at += op
    y = np.concatenate(out)
    ref = g["pll_y_ops" if name == "pll" else "cpll_y_ops"]
    assert not same(ref[3001:3100], g["pll_y" if name == "pll" else "cpll_y"][3001:3100]), "the reset shows nothing here"
    held(f"{name} reset", y, ref, r["bar"], r["S"], "restatement")


def test_meteor_costas_restatement_set_broken_modulation_and_reset():
    g = load("costas")
    assert parse_ops(g["ops"]) == M.COSTAS_OPS == [4000, "b1", 4000, "r", 4000] and M.SWITCH_AT == 4000
    r = M.loop_ref_and_S("meteor_costas_switch")
    assert same(g["x_broken"], r["x"]) and r["bar"] < 0.01 * RADIUS
    xr, xi = parts(r["x"])
    pcl = M.Pcl(1, M.COSTAS_BW)
    y = [c64(M.meteor_costas_run(pcl, xr[:, :4000], xi[:, :4000], False, M.trig64)),
         c64(M.meteor_costas_run(pcl, xr[:, 4000:8000], xi[:, 4000:8000], True, M.trig64))]
    assert same(np.concatenate(y), r["ref"][:8000])              # the switched restatement of the case, to the reset
    pcl.reset()
    y.append(c64(M.meteor_costas_run(pcl, xr[:, 8000:], xi[:, 8000:], True, M.trig64)))
    held("meteor_costas switch, reset", np.concatenate(y), g["ops_y"], r["bar"], r["S"], "restatement")


# ------------------------------------------------------------- CPU: the demodulator
@pytest.mark.parametrize("name", ["qpsk", "broken", "oqpsk", "ops"])
def test_meteor_restatement_reproduces_the_reference(name):
    r = M.meteor_ref_and_S(name)                                 # (asserts that the two restatements agree on every count)
    if name == "ops":
        g = load("demod_ops")
        x, want, counts, ops = g["x"], g["y"], g["counts"], parse_ops(g["ops"])
        assert ops == M.METEOR_OPS and int(g["seed"]) == M.METEOR_SEEDS["ops"][0]
        assert same(np.array(g["args"]), np.array(M.meteor_case("ops")[1], np.float64))
        got_counts = r["counts"]
    else:
        g = load("demod")
        x, want, counts = g[f"{name}_x"], g[f"{name}_y"], g[f"{name}_cut_counts"]
        assert same(np.array(g[f"{name}_args"]), np.array(M.meteor_args(*M.METEOR_CASES[name]), np.float64))
        got_counts, cut = M.ref_meteor(x, M.meteor_args(*M.METEOR_CASES[name]), M.trig64, CUTS)
        assert same(cut, r["ref"]), "the restatement in cuts differs from one call"
    assert same(x, r["x"]), "the fixture's input is not the case's first seed"
    print(f"meteor {name}: MM margin {r['margin']:.3e} (needs > {M.MM_MARGIN:.1e}), {len(want)} symbols")
    assert r["margin"] > M.MM_MARGIN, "an MM decision sits on a boundary: choose another seed"
    assert r["bar"] < 0.01 * RADIUS, "a bar above 1 % of the radius shows nothing"
    assert np.array_equal(got_counts, counts), f"differing counts: {np.count_nonzero(got_counts != counts)} (allowed: 0)"
    for kind in ("ref", "ref32"):
        held(f"meteor {name} {kind}", r[kind], want, r["bar"], r["S"], "restatement")


@pytest.mark.skipif(not have_reference(), reason="reference tree not mounted (GPU box): the committed fixtures cover it")
def test_a_fresh_probe_build_reproduces_the_committed_fixtures():
    assert_live_probe_reproduces("ref_meteor_", "meteor_fixtures")


# ------------------------------------------------------------------ gpu: the device blocks
@pytest.fixture()
def need_gpu():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: gpu tests need an MI355X"


def in_calls(block, x, cuts=CUTS):
    out, counts, i = [], [], 0
    for c in cuts:
        out.append(block.process(x[i:i + c]))
        counts.append(len(out[-1]))
        i += c
    assert i == len(x)
    return np.concatenate(out), np.array(counts, np.int32)


DEVICE_LOOPS = {
    "pll": lambda: dsp.PLL(M.LOOP_BW, 0.0, 0.0, -PI, PI),
    "carrier_pll": lambda: dsp.CarrierPLL(M.LOOP_BW, 0.0, 0.0, -PI, PI),
    "meteor_costas_plain": lambda: dsp.MeteorCostas(M.COSTAS_BW, False, 0.0, 0.0, -PI, PI),
    "meteor_costas_broken": lambda: dsp.MeteorCostas(M.COSTAS_BW, True, 0.0, 0.0, -PI, PI),
}


@gpu
@pytest.mark.parametrize("name", sorted(LOOPS))
def test_device_loops_against_the_reference(name, need_gpu):
    fname, key, case = LOOPS[name]
    g, r = load(fname), M.loop_ref_and_S(case)
    y = DEVICE_LOOPS[name]().process(r["x"])
    z, _ = in_calls(DEVICE_LOOPS[name](), r["x"])
    assert same(y, z), f"{name}: the stream in calls differs from one call"
    held(f"{name} device", y, g[key], r["bar"], r["S"], "device")


@gpu
@pytest.mark.parametrize("name", ["pll", "carrier_pll"])
def test_device_loops_reset_against_the_reference(name, need_gpu):
    g, r = load("loops"), M.loop_ref_and_S(name)
    b, out, at = DEVICE_LOOPS[name](), [], 0
    for op in M.LOOP_OPS:
        if op == "r":
            b.reset()
            continue
        out.append(b.process(r["x"][at:at + op]))
        at += op
    held(f"{name} reset device", np.concatenate(out), g["pll_y_ops" if name == "pll" else "cpll_y_ops"], r["bar"], r["S"], "device")


@gpu
def test_device_meteor_costas_set_broken_modulation_and_reset_against_the_reference(need_gpu):
    g, r = load("costas"), M.loop_ref_and_S("meteor_costas_switch")
    b, x = dsp.MeteorCostas(M.COSTAS_BW, False), r["x"]
    y = [b.process(x[:4000])]
    b.set_broken_modulation(True)
    y.append(b.process(x[4000:8000]))
    b.reset()
    y.append(b.process(x[8000:]))
    held("meteor_costas switch, reset device", np.concatenate(y), g["ops_y"], r["bar"], r["S"], "device")


@gpu
@pytest.mark.parametrize("name", ["qpsk", "broken", "oqpsk"])
def test_device_meteor_against_the_reference(name, need_gpu):
    g, r = load("demod"), M.meteor_ref_and_S(name)
    make = lambda: dsp.Meteor(*M.meteor_args(*M.METEOR_CASES[name]))
    y = make().process(r["x"])
    z, counts = in_calls(make(), r["x"])
    assert same(y, z), f"meteor {name}: the stream in calls differs from one call"
    want = g[f"{name}_cut_counts"]
    assert np.array_equal(counts, want), f"differing counts: {np.count_nonzero(counts != want)} (allowed: 0)"
    held(f"meteor {name} device", y, g[f"{name}_y"], r["bar"], r["S"], "device")


@gpu
def test_device_meteor_setters_and_reset_against_the_reference(need_gpu):
    g, r = load("demod_ops"), M.meteor_ref_and_S("ops")
    b, o = M.OPS_START
    m, out, counts, at = dsp.Meteor(*M.meteor_args(b, o)), [], [], 0
    for op in M.METEOR_OPS:
        if op == "r":
            m.reset()
        elif isinstance(op, str):
            (m.set_broken_modulation if op[0] == "b" else m.set_oqpsk)(op[1] == "1")
        else:
            out.append(m.process(r["x"][at:at + op]))
            counts.append(len(out[-1]))
            at += op
    want = g["counts"]
    assert np.array_equal(counts, want), f"differing counts: {np.count_nonzero(np.array(counts) != want)} (allowed: 0)"
    held("meteor ops device", np.concatenate(out), g["y"], r["bar"], r["S"], "device")
