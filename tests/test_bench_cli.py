"""bench.py's command line: a plain run times --config only and prints its line, --full adds the parts
that take runs of their own, --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("configs", "per_call", "spectrum_ulp", "spectrum_f64_mode_cost", "cpu_baseline", "speedup_vs_cpu_all_cores")


def test_parse_plain_full_and_dump():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2) and a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "d", "--no-cpu"])
    assert a.full is True and a.dump_outputs == "d" and a.no_cpu is True


def test_dump_plan_default_c5_sizes():
    """The default C5 step: the waterfall rows, the VFO output and the audio whole, the 2^28 dB bins as a
    sample at sorted positions that only depend on the array's length; under 64 MB of float32 in all."""
    sizes = {"spectra": 1 << 28, "waterfall_rows": 1 << 23, "vfo_iq": 1 << 21, "audio_stereo": 1 << 21}
    plan = bench.dump_plan(sizes)
    assert plan["waterfall_rows"] is None and plan["vfo_iq"] is None and plan["audio_stereo"] is None
    pos = plan["spectra"]
    assert pos.dtype == np.int64 and pos.size == bench.DUMP_SAMPLE
    assert pos.min() >= 0 and pos.max() < 1 << 28 and np.all(np.diff(pos) >= 0)
    assert len(np.unique(pos // 65536)) == 4096          # every frame of the step is sampled
    np.testing.assert_array_equal(pos, bench.dump_plan({"other_name": 1 << 28})["other_name"])
    written = sum(sizes[n] if p is None else p.size for n, p in plan.items())
    assert 4 * written <= 64 * 10**6


def test_dump_plan_shrinks_to_the_cap():
    sizes = {"a": 1 << 23, "b": 1 << 23, "c": 1 << 23, "d": 1 << 30, "e": 100}
    plan = bench.dump_plan(sizes)
    written = sum(sizes[n] if p is None else p.size for n, p in plan.items())
    assert 4 * written <= 64 * 10**6 and plan["e"] is None and plan["d"].max() < 1 << 30


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR` on a 4-frame batch: one JSON line without
    the --full parts, and DIR holds the last step's outputs: the dB rows against the fp64 truth of the same
    seeded input and the RxVFO output against the oracle's fourth block at the smoke run's bars, every
    waterfall row exactly fft_scaler's zoom of its dB row."""
    import oracle
    import torch
    from sdrpp_amd import dsp
    d = tmp_path / "out"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--log2-batch", "18", "--dump-outputs", str(d)], env=env, capture_output=True, text=True,
                       timeout=240, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["metric"] == bench.METRIC and r["unit"] == "MS/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
    assert r["steps"] == 3 and r["ms_per_step"] > 0
    assert abs(r["value"] - (1 << 18) / (r["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * r["value"]
    assert not [k for k in FULL_ONLY if k in r]

    N, frames, zw = 65536, 4, 2048
    out = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert sorted(out) == ["audio_stereo", "spectra", "vfo_iq", "waterfall_rows"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in out.values())
    assert sum(v.nbytes for v in out.values()) <= 64 * 10**6
    x = bench.CudaRuntime().rand(2 * frames * N, 0xACE1).cpu().numpy().view(np.complex64)
    rows = out["spectra"].reshape(frames, N)
    w = dsp.create_window(6, N)
    for j in range(frames):
        X = np.fft.fft((x[j * N:(j + 1) * N] * w).astype(np.complex64).astype(np.complex128))
        ref = 10 * np.log10(X.real ** 2 + X.imag ** 2)
        sel = ref > ref.max() - 60
        assert np.abs(rows[j][sel] - ref[sel]).max() < 1e-3
        np.testing.assert_array_equal(out["waterfall_rows"].reshape(frames, zw)[j], oracle.zoom(rows[j], 0.0, 1.0, 1.0, zw))
    vfo = oracle.RxVFO(61.44e6, 240000, 200000, 2.5e6)
    for _ in range(4):                                   # warm-up + 3 timed steps of the same batch
        ref_iq = vfo.process(x)
    got = out["vfo_iq"].view(np.complex64)
    assert len(got) == len(ref_iq) == frames * N // 256 and np.abs(got - ref_iq).max() < 5e-5
    assert out["audio_stereo"].size > 0 and out["audio_stereo"].size % 2 == 0
