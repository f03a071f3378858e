"""Shared parity helpers (tolerances are stated here, once)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

EPS32 = np.finfo(np.float32).eps


def fir_atol(taps, x):
    """fp32 FIR vs fp64-accumulated oracle: |err| <= 8*eps32*sqrt(ntaps)*sum|h|*max|x| (+tiny)."""
    h = np.abs(np.asarray(taps)).sum()
    xm = np.abs(np.asarray(x)).max() if np.size(x) else 1.0
    return 8 * EPS32 * np.sqrt(len(taps)) * h * xm + 1e-30


def assert_close_c(a, b, atol, what=""):
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    err = np.abs(a.astype(np.complex128) - b.astype(np.complex128)).max() if a.size else 0.0
    assert err <= atol, f"{what}: max abs err {err:.3e} > atol {atol:.3e}"
    return err


def db_check(db_gpu, power_true, N, ref32_db=None, floor_db=60.0):
    """Spectrum parity (DESIGN.md §4 'Parity bar'), on bins within `floor_db` of the frame peak.
    With a reference-class fp32 FFT (pocketfft single precision) on the same windowed frame:
    1. rms dB error <= 2x its rms (+ the rms of 1 ulp of the fp32 dB values);
    2. per bin, in fp32 ulps of the correctly rounded dB of the exact DFT (db_ulp_errors), against
       pocketfft's ulps on the SAME frame (round 4; replaces round 3's 8x ratio of two single-bin dB
       maxima): within-1-ulp fraction >= pocketfft's - 1 point and p99.9 <= pocketfft's + 4 ulp
       (frames with >= 1000 bins in range). Measured over the 510-frame corpus (corpus_ulp_rows,
       profiles/r4/spectrum_corpus_*.json): fraction -0.59 points at worst, p99.9 +3 ulp;
    3. worst bin, per frame, in magnitude: every | |X_gpu,k| - |X_true,k| | <= 2x pocketfft's worst on
       the same frame + the magnitude step of one fp32 ulp of that bin's dB value (measured r4d: at most
       1.33x over 30 random frames, 64 to 1M points). The worst bin in dB ulps is not a per-frame bar:
       it is set by the smallest in-range bins (the absolute error divided by a bin 60 dB down), a
       heavy-tailed statistic -- r4b: a 64k frame at 102 ulp where pocketfft's worst was 21 ulp, while
       its fraction, p99.9 and rms matched pocketfft's. The ulp worst bin is bounded over the corpus
       instead (test_spectrum_ulp_corpus: <= 1.25x pocketfft's worst over all frames of a size);
    4. normwise: || |X_gpu| - |X_true| ||_2 <= 4 * eps32 * log2(N) * ||X_true||_2 (all bins).
    Without a reference-class FFT the bound is 2e-4 dB."""
    db_true = 10.0 * np.log10(np.maximum(power_true, 1e-300))
    peak = db_true.max()
    sel = db_true >= peak - floor_db
    err = np.abs(db_gpu.astype(np.float64) - db_true)[sel]
    ulp = np.spacing(np.abs(db_gpu[sel]).astype(np.float32)).astype(np.float64)
    if ref32_db is not None:
        rerr = np.abs(ref32_db.astype(np.float64) - db_true)[sel]
        rms_g, rms_r = np.sqrt(np.mean(err ** 2)), np.sqrt(np.mean(rerr ** 2))
        # + the rms of 1 ulp of the fp32 dB value: the reference writes 10*log10f(re^2+im^2) in
        # fp32 (volk_32fc_s32f_power_spectrum_32f), i.e. the dB row itself carries ~1 ulp
        # (log10f + the x10 rounding); the scipy row here is rounded once from fp64
        ulp_rms = np.sqrt(np.mean(ulp ** 2))
        assert rms_g <= 2.0 * rms_r + ulp_rms + 1e-12, f"rms dB err {rms_g:.3e} > 2 x fp32-ref {rms_r:.3e} + ulp {ulp_rms:.3e}"
        eg, er = db_ulp_errors(db_gpu, power_true, floor_db), db_ulp_errors(ref32_db, power_true, floor_db)
        sg, sr = ulp_stats(eg), ulp_stats(er)
        if eg.size >= 1000:
            assert sg["frac_le_1ulp"] >= sr["frac_le_1ulp"] - 0.01, (sg, sr)
            assert sg["p999"] <= sr["p999"] + 4.0, (sg, sr)
        mt = np.sqrt(np.asarray(power_true, np.float64))[sel]
        dg = np.abs(np.sqrt(10.0 ** (db_gpu.astype(np.float64)[sel] / 10.0)) - mt)
        ar = np.abs(np.sqrt(10.0 ** (ref32_db.astype(np.float64)[sel] / 10.0)) - mt).max()
        # per bin, the magnitude step of one fp32 ulp of its dB value (the row's own quantisation:
        # tonal frames with a few bins in range sit at it, r4b C1 frames: 1 ulp both, 2.4x in magnitude)
        q = mt * (np.log(10.0) / 20.0) * np.spacing(np.abs(db_true[sel]).astype(np.float32)).astype(np.float64)
        write_report("spectrum_worst_bin", {"N": int(N), "bins": int(eg.size), "ulp_gpu": sg, "ulp_pocketfft": sr,
                                            "abs_gpu": float(dg.max()), "abs_pocketfft": float(ar),
                                            "excess_over_q": float((dg - q).max())})
        assert np.all(dg <= 2.0 * ar + q), (float(dg.max()), float(ar), float((dg - q).max()), sg, sr)
    else:
        assert np.all(err <= np.maximum(2e-4, 2.0 * ulp)), f"max dB err {err.max():.3e}"
    mag_gpu = np.sqrt(10.0 ** (db_gpu.astype(np.float64) / 10.0))
    mag_true = np.sqrt(power_true)
    nerr = np.linalg.norm(mag_gpu - mag_true) / np.linalg.norm(mag_true)
    assert nerr <= 4 * EPS32 * np.log2(N), f"normwise magnitude error {nerr:.3e}"
    return err.max(), nerr


def ulp_stats(e):
    return {"frac_le_1ulp": float(np.mean(e <= 1.0)), "p999": float(np.percentile(e, 99.9)), "max": float(e.max())}


def corpus_frame(N, nz, wt, k):
    """Seed-fixed random frame k of the spectrum corpus (depends only on N, window, k)."""
    rng = np.random.default_rng(1234 + wt + 100 * k + 7 * N)
    return (rng.uniform(-1, 1, nz) + 1j * rng.uniform(-1, 1, nz)).astype(np.complex64)


def corpus_ulp_rows(frames=24, f1m=6, sizes=(4096, 16384, 65536)):
    """The spectrum accuracy corpus: sizes x the 7 window types x `frames` random frames, plus `f1m`
    1M-point frames (nz = 1e6, BH7). Per frame: the GPU's (fp32 kernels and fp64-interior mode) and
    pocketfft's ulp statistics against the fp64 truth (bins within 60 dB of the peak)."""
    import oracle
    from sdrpp_amd import dsp
    cases = [(N, N, wt, k) for N in sizes for wt in range(7) for k in range(frames)]
    cases += [(1 << 20, 1000000, 6, k) for k in range(f1m)]
    plans, rows = {}, []
    for N, nz, wt, k in cases:
        if (N, nz, wt) not in plans:
            plans[(N, nz, wt)] = (dsp.FFTSpectrum(N, nz, wt), dsp.FFTSpectrum(N, nz, wt, precision="f64"))
        f32, f64 = plans[(N, nz, wt)]
        x = corpus_frame(N, nz, wt, k)
        w = oracle.create_window(wt, nz)
        truth = oracle.fft_truth_power(x, nz, N, w)
        e = db_ulp_errors(f32.logmag(x), truth)
        er = db_ulp_errors(ref32_fft_db(x, nz, N, w), truth)
        e64 = db_ulp_errors(f64.logmag(x), truth)
        g, r = ulp_stats(e), ulp_stats(er)
        rows.append({"N": N, "nz": nz, "w": wt, "k": k, "bins": int(e.size), "gpu": g, "pocketfft": r,
                     "max_ratio": g["max"] / max(r["max"], 1.0), "f64_max": float(e64.max()),
                     "f64_frac_exact": float(np.mean(e64 == 0))})
    return rows


def corpus_aggregate(rows):
    agg = {}
    for N in sorted({r["N"] for r in rows}):
        rs = [r for r in rows if r["N"] == N]
        agg[str(N)] = {
            "frames": len(rs),
            "gpu_min_frac_le_1ulp": min(r["gpu"]["frac_le_1ulp"] for r in rs),
            "pocketfft_min_frac_le_1ulp": min(r["pocketfft"]["frac_le_1ulp"] for r in rs),
            "min_frac_diff": min(r["gpu"]["frac_le_1ulp"] - r["pocketfft"]["frac_le_1ulp"] for r in rs),
            "gpu_max_p999": max(r["gpu"]["p999"] for r in rs),
            "pocketfft_max_p999": max(r["pocketfft"]["p999"] for r in rs),
            "max_p999_diff": max(r["gpu"]["p999"] - r["pocketfft"]["p999"] for r in rs),
            "gpu_max": max(r["gpu"]["max"] for r in rs),
            "pocketfft_max": max(r["pocketfft"]["max"] for r in rs),
            "gpu_mean_frame_max": float(np.mean([r["gpu"]["max"] for r in rs])),
            "pocketfft_mean_frame_max": float(np.mean([r["pocketfft"]["max"] for r in rs])),
            "frames_max_ratio_gt_1.25": sum(r["max_ratio"] > 1.25 for r in rs),
            "worst_max_ratio": max(r["max_ratio"] for r in rs),
            "f64_max": max(r["f64_max"] for r in rs),
            "f64_min_frac_exact": min(r["f64_frac_exact"] for r in rs),
        }
    return agg


def db_ulp_errors(db, power_true, floor_db=60.0):
    """|db - db_true| in units of the fp32 ulp of the true dB value (db_true = 10 log10 of the fp64
    power, rounded once to fp32), on bins within `floor_db` of the frame peak. This is the
    north_star's "<= 1 ulp on FFT magnitude" measured literally: a value of 1 means the dB row is
    one fp32 step from the correctly rounded dB of the exact DFT."""
    t64 = 10.0 * np.log10(np.maximum(np.asarray(power_true, np.float64), 1e-300))
    sel = t64 >= t64.max() - floor_db
    t32 = t64[sel].astype(np.float32)
    ulp = np.spacing(np.abs(t32)).astype(np.float64)
    return np.abs(np.asarray(db, np.float32)[sel].astype(np.float64) - t32.astype(np.float64)) / ulp


def ulp_summary(e):
    return {"bins": int(e.size), "p50": float(np.percentile(e, 50)), "p90": float(np.percentile(e, 90)),
            "p99": float(np.percentile(e, 99)), "max": float(e.max()), "frac_le_1ulp": float(np.mean(e <= 1.0))}


def write_report(name, obj):
    """Append a JSON line to $SDRGPU_REPORT_DIR/<name>.jsonl when that directory is set (GPU
    sessions copy these into profiles/)."""
    import json
    d = os.environ.get("SDRGPU_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name + ".jsonl"), "a") as f:
            f.write(json.dumps(obj) + "\n")


def ref32_fft_db(x, nz, N, window):
    """A reference-class fp32 FFT (pocketfft single precision via scipy) on the windowed frame."""
    import scipy.fft
    buf = np.zeros(N, dtype=np.complex64)
    buf[:nz] = (np.asarray(x[:nz], dtype=np.complex64) * np.asarray(window, dtype=np.float32)).astype(np.complex64)
    X = scipy.fft.fft(buf, workers=1)
    assert X.dtype == np.complex64
    p = X.real.astype(np.float32) ** 2 + X.imag.astype(np.float32) ** 2
    with np.errstate(divide="ignore"):
        return (10.0 * np.log10(p.astype(np.float64))).astype(np.float32)


def iq(rng, n, scale=1.0):
    """SpeedTester-style uniform [-1,1) complex IQ (core/src/dsp/bench/speed_tester.h:37-41)."""
    return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64) * np.float32(scale)


def two_pass_fft(N, nz, window=6):
    """An FFTSpectrum on the two-pass launches of the 64k plan: the front end's transform (its plans are
    two-pass, frontend.hip fe_update_fft), which its rows are checked against bit for bit."""
    from sdrpp_amd import dsp
    keys = ("SDRGPU_TUNING", "SDRGPU_FFT_1P")
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update(SDRGPU_TUNING="1", SDRGPU_FFT_1P="0")
    try:
        return dsp.FFTSpectrum(N, nz, window)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_generator = []


def ref_generator():
    """tools/gen_ref_fixtures.py as a module (loaded once)."""
    if not _generator:
        import importlib.util
        path = os.path.join(os.path.dirname(GOLDEN), "..", "tools", "gen_ref_fixtures.py")
        spec = importlib.util.spec_from_file_location("gen_ref_fixtures", path)
        _generator.append(importlib.util.module_from_spec(spec))
        spec.loader.exec_module(_generator[0])
    return _generator[0]


def have_reference():
    """The one skip condition of the live-probe tests: the reference's dsp headers and the Meteor module's."""
    return ref_generator().have_reference()


def assert_live_probe_reproduces(prefix, fixtures):
    """A fresh build of the reference probes reproduces every committed tests/golden/<prefix>*.npz: the same files,
    the same keys, and per array the same dtype, shape and bytes. `fixtures` names the generator's function."""
    import subprocess
    gen = ref_generator()
    subprocess.check_call(["make", "-C", os.path.join(gen.ROOT, "oracle"), "-s", "ref"])
    files = getattr(gen, fixtures)()
    assert sorted(files) == sorted(f for f in os.listdir(GOLDEN) if f.startswith(prefix))
    for fname, arrays in files.items():
        assert os.path.getsize(os.path.join(GOLDEN, fname)) <= gen.MAX_BYTES, fname
        g = np.load(os.path.join(GOLDEN, fname))
        assert sorted(g.files) == sorted(arrays), fname
        for k, v in arrays.items():
            v = np.asarray(v)
            assert g[k].dtype == v.dtype and g[k].shape == v.shape and g[k].tobytes() == v.tobytes(), f"{fname}: {k}"
