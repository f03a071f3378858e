"""Call times of the broadcast-FM banks against the same work on single-stream handles (needs an MI355X):
    python tools/time_wfm_banks.py [out.json] [case ...]      (default profiles/r18/bank_wfm_time.json, every case)
    python tools/time_wfm_banks.py [out.json] --split DIR     (the launches of one call from a kernel trace, below)
The shape and the timing of tools/time_rate_banks.py: S = 1024 streams of 1024 frames at 240 kS/s on device-resident
buffers, device events, one warm-up call and 5 timed ones, the median with min and max.
  cfir305_f32 / _c64   BankFIRComplex with the 305 pilot taps, float32 / complex64 rows in, in both forms of its kernel
                       (bank_wfm_kernels.h): tiled (bank_ms) and direct (direct_ms), chosen at creation through
                       SDRGPU_TUNING=1 SDRGPU_BANK_CFIR_TILED=1 | 0
  stereo_decoder       BankStereoDecoder on the MPX that BankQuadrature makes of the input, in both forms of its pilot filter
  broadcast_fm_stereo / _mono   BankBroadcastFM (low-pass on), in both forms, against 1024 dsp.BroadcastFM(stereo=True |
                       False) handles fed their columns back to back: the way to do this work without the bank
The input is a stereo broadcast per stream (tests/_bank_wfm.py stereo_stream: own tones, phases and amplitude), so the
PLLs lock as they do in use. Recorded, not tuned: a bank that is not below its handles figure is listed ("not_faster").
--split DIR: DIR holds the kernel trace (csv) of `rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python
tools/time_wfm_banks.py x.json stereo_decoder`. The median duration of every kernel of the decoder's call goes to
"decoder_launches_us": the pilot filter, the PLL walk alone (bank_pll_kernel), the matrix, the two history carries."""
import contextlib
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

FS, DEVIATION = 240000.0, 100000.0
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r18", "bank_wfm_time.json")


@contextlib.contextmanager
def form(tiled):
    keys = ("SDRGPU_TUNING", "SDRGPU_BANK_CFIR_TILED")
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update(SDRGPU_TUNING="1", SDRGPU_BANK_CFIR_TILED="1" if tiled else "0")
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def load(out):
    rec = {"cases": {}}
    if os.path.exists(out):                                     # (cases may be measured in several runs)
        with open(out) as f:
            rec = json.load(f)
    return rec


def save(out, rec):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def split(out, trace_dir):
    """the per-kernel medians of the stereo decoder's call from a rocprofv3 kernel trace"""
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert paths, f"no kernel trace under {trace_dir}"
    names = {"bank_cfir_tiled": "pilot_fir_tiled", "bank_cfir_direct": "pilot_fir_direct", "bank_pll_kernel": "pll_walk",
             "bank_stereo_matrix": "matrix", "fir_hist": "history_carry", "bank_quad": "quadrature"}
    us = {}
    for p in paths:
        with open(p) as f:
            for row in csv.DictReader(f):
                for key, label in names.items():
                    if key in row["Kernel_Name"]:
                        us.setdefault(label, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    rec = load(out)
    rec["decoder_launches_us"] = {k: {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                                      "launches": len(v)} for k, v in sorted(us.items())}
    save(out, rec)
    for k, v in rec["decoder_launches_us"].items():
        print(f"{k}: {v['median']} us [{v['min']}, {v['max']}] over {v['launches']} launches")


def main():
    args = sys.argv[1:]
    out = args[0] if args and args[0].endswith(".json") else DEFAULT_OUT
    if "--split" in args:
        return split(out, args[args.index("--split") + 1])
    import torch
    import sdrpp_amd
    from sdrpp_amd import dsp
    from time_banks import S, FRAMES, TIMED, summary
    from time_audio_banks import timed
    from _bank_wfm import stereo_stream
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: this timing needs an MI355X"
    names = [a for a in args if not a.endswith(".json")] or ["cfir305_f32", "cfir305_c64", "stereo_decoder", "broadcast_fm_stereo",
                                                             "broadcast_fm_mono"]
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    pilot = dsp.band_pass(18750, 19250, 3000, FS, odd=True, complex_taps=True)
    assert len(pilot) == 305
    # stream k's broadcast repeats with k mod 130 (the streams of the tests); the time does not depend on the data
    cols = np.stack([stereo_stream(k, FRAMES, FS) for k in range(130)])
    x = np.ascontiguousarray(cols[np.arange(S) % 130].T)                                       # (FRAMES, S) complex64
    d_iq = torch.from_numpy(x.view(np.float32).reshape(FRAMES, S, 2)).cuda()
    d_cols = d_iq.permute(1, 0, 2).contiguous()
    d_mpx = torch.empty(S * FRAMES, dtype=torch.float32, device="cuda")
    d_out = torch.empty(2 * S * FRAMES, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    q = dsp.BankQuadrature(S, 2.0 * np.pi * (DEVIATION / FS))
    q.process_dev(d_iq.data_ptr(), FRAMES, d_mpx.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    q.close()
    # name: (bank(S), its device input, bytes in + out per call, the single-stream handle or None)
    cases = {
        "cfir305_f32": (lambda: dsp.BankFIRComplex(S, pilot, real_input=True), d_mpx, 12, None),
        "cfir305_c64": (lambda: dsp.BankFIRComplex(S, pilot), d_iq, 16, None),
        "stereo_decoder": (lambda: dsp.BankStereoDecoder(S, FS), d_mpx, 12, None),
        "broadcast_fm_stereo": (lambda: dsp.BankBroadcastFM(S, DEVIATION, FS), d_iq, 16, lambda: dsp.BroadcastFM(DEVIATION, FS, True, stereo=True)),
        "broadcast_fm_mono": (lambda: dsp.BankBroadcastFM(S, DEVIATION, FS, stereo=False), d_iq, 16,
                              lambda: dsp.BroadcastFM(DEVIATION, FS, True, stereo=False)),
    }
    rec = load(out)
    rec.update({"streams": S, "frames": FRAMES, "samplerate": FS, "timed_calls": TIMED})
    for name in names:
        make_bank, d_in, bytes_per, make_single = cases[name]
        ms = {}
        for tiled in (True, False):
            with form(tiled):
                bank = make_bank()
            ms[tiled] = timed(stream, lambda: bank.process_dev(d_in.data_ptr(), FRAMES, d_out.data_ptr(), stream.cuda_stream))
            bank.close()
        handles_ms = None
        if make_single:
            handles = [make_single() for _ in range(S)]

            def all_handles():
                for k, h in enumerate(handles):
                    h.process_dev(d_cols.data_ptr() + k * FRAMES * 8, FRAMES, d_out.data_ptr() + k * FRAMES * 8, stream.cuda_stream)
            handles_ms = timed(stream, all_handles)
            for h in handles:
                h.close()
        r = summary(ms[True], handles_ms if handles_ms else ms[True])
        if not handles_ms:
            for k in ("handles_ms", "handles_ms_median", "handles_over_bank"):
                r.pop(k)
        d = float(np.median(ms[False]))
        r.update({"direct_ms": [round(v, 4) for v in ms[False]], "direct_ms_median": round(d, 4),
                  "direct_over_tiled": round(d / r["bank_ms_median"], 2), "bytes_in_plus_out": bytes_per * S * FRAMES})
        rec["cases"][name] = r
        print(f"{name}: tiled {r['bank_ms_median']:.3f} ms [{min(ms[True]):.3f}, {max(ms[True]):.3f}], direct {d:.3f} ms "
              f"[{min(ms[False]):.3f}, {max(ms[False]):.3f}]"
              + (f", 1024 handles {r['handles_ms_median']:.2f} ms [{min(handles_ms):.2f}, {max(handles_ms):.2f}], x{r['handles_over_bank']}"
                 if handles_ms else ""), flush=True)
        rec["not_faster"] = [n for n, c in rec["cases"].items()
                             if "handles_ms_median" in c and not max(c["bank_ms_median"], c["direct_ms_median"]) < c["handles_ms_median"]]
        save(out, rec)


if __name__ == "__main__":
    main()
