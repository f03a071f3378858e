"""tests/golden/ref_meteor_*.npz: the reference's loop::PLL, loop::CarrierTrackingPLL, loop::MeteorCostas and
demod::Meteor run from its own headers by tools/ref_meteor_probe.cpp. Run where the reference tree exists; the
fixtures are committed so that a machine without it checks against them.

The probe is compiled into a temporary directory (never into the repository) with the reference tree on the
include path and oracle/ref_standins.cpp (read, not modified) linked in. Each file holds the inputs, the
parameters, the call lists, the per-call counts and the outputs. `fixtures()` builds them in memory;
tests/test_meteor_ref.py calls it to require that a fresh build reproduces the committed files.

    python tools/gen_meteor_fixtures.py            write the fixtures
    python tools/gen_meteor_fixtures.py --search   print, per demodulator case, seeds that meet the case's precondition
                                                   (tests/_meteor.py METEOR_SEEDS: the two restatements agree on every count
                                                   and MM decision; first the seed with the widest MM margin)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SDRPP_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 709691          # as tools/gen_ref_fixtures.py
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def have_reference():
    return os.path.isdir(os.path.join(REF, "core", "src", "dsp")) and \
        os.path.isfile(os.path.join(REF, "decoder_modules", "meteor_demodulator", "src", "meteor_demod.h"))


def build_probe(tmp):
    exe = os.path.join(tmp, "ref_meteor_probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math",
                           "-I" + os.path.join(REF, "core", "src"), "-I" + os.path.join(ROOT, "oracle", "ref_fmt"),
                           "-I" + os.path.join(ROOT, "tests", "stubs"),
                           "-I" + os.path.join(REF, "decoder_modules", "meteor_demodulator", "src"), "-w",
                           os.path.join(ROOT, "tools", "ref_meteor_probe.cpp"), os.path.join(ROOT, "oracle", "ref_standins.cpp"),
                           "-o", exe, "-lpthread"])
    return exe


def num(v):
    return v if isinstance(v, str) else (str(int(v)) if isinstance(v, (bool, int, np.integer)) else f"{float(v):.17g}")


def probe(exe, mode, calls, params, x):
    """One run: (int32 counts per process() call, complex64 outputs); the framing of gen_ref_fixtures.py's blocks()."""
    raw = subprocess.run([exe, mode, ",".join(num(c) for c in calls), *map(num, params)],
                         input=np.ascontiguousarray(x, np.complex64).tobytes(), capture_output=True, check=True).stdout
    nc = int(np.frombuffer(raw[:4], np.int32)[0])
    counts = np.frombuffer(raw[4:4 + 4 * nc], np.int32)
    y = np.frombuffer(raw[4 + 4 * nc:], np.complex64)
    assert len(y) == int(counts.sum())
    return counts, y


def whole_and_cut(exe, mode, params, x, cuts):
    """The reference fed in one call and in `cuts`: the same outputs, kept once, and the cut feed's counts."""
    cw, yw = probe(exe, mode, [len(x)], params, x)
    cc, yc = probe(exe, mode, cuts, params, x)
    assert yw.tobytes() == yc.tobytes() and int(cw[0]) == int(cc.sum()), mode
    return yw, cc


def fixtures(exe):
    """{file name: {key: array}} of every ref_meteor_*.npz."""
    import _meteor as M
    from _restated import CUTS, N
    PI = float(M.FL_M_PI)
    files = {}

    g = {"cuts": np.array(CUTS, np.int32), "ops": np.array(",".join(map(str, M.LOOP_OPS)))}
    g["params"] = np.array([M.LOOP_BW, 0.0, 0.0, -PI, PI])
    g["x"] = x = M.carrier(0)
    for mode in ("pll", "cpll"):
        g[f"{mode}_y"] = whole_and_cut(exe, mode, g["params"], x, CUTS)[0]
        g[f"{mode}_y_ops"] = probe(exe, mode, M.LOOP_OPS, g["params"], x)[1]
    files["ref_meteor_loops.npz"] = g

    g = {"cuts": np.array(CUTS, np.int32), "ops": np.array(",".join(map(str, M.COSTAS_OPS)))}
    g["params"] = np.array([M.COSTAS_BW, 0.0, 0.0, -PI, PI])   # bandwidth, then what follows `broken`
    for kind, broken in (("qpsk", 0), ("broken", 1)):
        g[f"x_{kind}"] = x = M.unit_lrpt(0, kind)
        p = [M.COSTAS_BW, broken, 0.0, 0.0, -PI, PI]
        g[f"{kind}_y"] = whole_and_cut(exe, "mcostas", p, x, CUTS)[0]
    # the broken-modulation signal through a loop that starts with the plain error
    g["ops_y"] = probe(exe, "mcostas", M.COSTAS_OPS, [M.COSTAS_BW, 0, 0.0, 0.0, -PI, PI], g["x_broken"])[1]
    files["ref_meteor_costas.npz"] = g

    g = {"cuts": np.array(CUTS, np.int32)}
    for name in M.METEOR_CASES:
        xs, args, _ = M.meteor_case(name)
        g[f"{name}_x"], g[f"{name}_args"], g[f"{name}_seed"] = xs[0], np.array(args, np.float64), np.array(M.METEOR_SEEDS[name][0])
        g[f"{name}_y"], g[f"{name}_cut_counts"] = whole_and_cut(exe, "meteor", args, xs[0], CUTS)
    files["ref_meteor_demod.npz"] = g

    xs, args, ops = M.meteor_case("ops")
    g = {"x": xs[0], "args": np.array(args, np.float64), "seed": np.array(M.METEOR_SEEDS["ops"][0]),
         "ops": np.array(",".join(map(str, ops)))}
    g["counts"], g["y"] = probe(exe, "meteor", ops, args, xs[0])
    files["ref_meteor_demod_ops.npz"] = g
    return files


def search(per_case=8, tries=48):
    import _meteor as M
    for name in M.METEOR_SEEDS:
        kind = M.OPS_KIND if name == "ops" else name
        b, o = M.OPS_START if name == "ops" else M.METEOR_CASES[name]
        ops = M.METEOR_OPS if name == "ops" else [M.N]
        good = []
        for s0 in range(0, tries, 8):
            seeds = list(range(s0, s0 + 8))
            xs = np.stack([M.lrpt_signal(s, kind)[0] for s in seeds])
            ca, ya, da = M.mm_margin(xs, M.meteor_args(b, o), ops, M.trig32)
            cb, yb, db = M.mm_margin(xs, M.meteor_args(b, o), ops, M.trig64)
            for k, s in enumerate(seeds):
                agree = np.array_equal(ca[k], cb[k]) and M.gap(ya[k], yb[k]) < 1e-5
                print(f"{name} seed {s}: margin {min(da[k], db[k]):.2e}{', the restatements agree' if agree else ''}", flush=True)
                if agree:
                    good.append((min(da[k], db[k]), s))
        first = max(good)[1]                                    # the widest margin first: the fixture's stream
        print(f'    "{name}": {[first] + [s for _, s in good if s != first][:per_case - 1]},   # margin {max(good)[0]:.2e}')


def main():
    if "--search" in sys.argv:
        return search()
    assert have_reference(), f"no reference tree at {REF}"
    with tempfile.TemporaryDirectory() as tmp:
        files = fixtures(build_probe(tmp))
    for fname, arrays in files.items():
        path = os.path.join(OUT, fname)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, f"{fname}: {size} bytes > {MAX_BYTES}"
        print(f"{fname}: {size} bytes")


if __name__ == "__main__":
    main()
