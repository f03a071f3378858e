"""Call times of the stream banks against the same work on single-stream handles (needs an MI355X):
    python tools/time_banks.py [out.json] [case ...]     (default profiles/r12/bank_time.json, every case)
S = 1024 streams of 1024 frames (2^20 samples in all) on device-resident buffers, per case:
* bank: one bank handle, one process_dev call on the (frames, S) buffer;
* handles: 1024 single-stream handles, handle k given its 1024-sample column (a stream-major copy of the
  same data) by process_dev, back to back on one stream -- what the library offered before the banks.
Both between two device events per call, one warm-up call and 5 timed ones; the 5 times are kept, the
summary is their median with min and max. The channelizer pair times sdrgpu_channelizer(1024) followed by
the GFSK bank on its device output; on the handles side the channelizer output has to be transposed to
stream-major first (a device transpose on the same stream, inside the timed region).
Recorded, not tuned. The one condition: every bank figure below its handles figure."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdrpp_amd  # noqa: E402
from sdrpp_amd import dsp  # noqa: E402

S = 1024
FRAMES = 1024
TIMED = 5
PSK = (4, 1.0, 4.0, 31, 0.6, 0.01, 0.005, 2.5e-5, 0.01, 0.01)
GFSK = (12000.0, 48000.0, 3000.0, 31, 0.6, 2.5e-5, 0.01, 0.01)
MM = (4.0, 2.5e-5, 0.01, 0.01)

# name: (bank(S), single-stream handle, complex input, bytes per output element)
CASES = {
    "fast_agc_float": (lambda: dsp.BankFastAGC(S, 1.0, 1e6, 0.1), lambda: dsp.FastAGC(1.0, 1e6, 0.1), False, 4),
    "fast_agc_complex": (lambda: dsp.BankFastAGC(S, 1.0, 1e6, 0.1, complex_data=True),
                         lambda: dsp.FastAGC(1.0, 1e6, 0.1, complex_data=True), True, 8),
    "costas_2": (lambda: dsp.BankCostas(S, 2, 0.005), lambda: dsp.Costas(2, 0.005), True, 8),
    "costas_4": (lambda: dsp.BankCostas(S, 4, 0.005), lambda: dsp.Costas(4, 0.005), True, 8),
    "costas_8": (lambda: dsp.BankCostas(S, 8, 0.005), lambda: dsp.Costas(8, 0.005), True, 8),
    "mm_float": (lambda: dsp.BankMM(S, *MM), lambda: dsp.MM(*MM), False, 4),
    "mm_complex": (lambda: dsp.BankMM(S, *MM, complex_data=True), lambda: dsp.MM(*MM, complex_data=True), True, 8),
    "psk": (lambda: dsp.BankPSK(S, *PSK), lambda: dsp.PSK(*PSK), True, 8),
    "gfsk": (lambda: dsp.BankGFSK(S, *GFSK), lambda: dsp.GFSK(*GFSK), True, 4),
}


def timed(stream, call):
    call()                                                       # warm-up
    stream.synchronize()
    ms = []
    for _ in range(TIMED):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def summary(bank_ms, handles_ms):
    b, h = float(np.median(bank_ms)), float(np.median(handles_ms))
    return {"bank_ms": [round(v, 4) for v in bank_ms], "handles_ms": [round(v, 3) for v in handles_ms],
            "bank_ms_median": round(b, 4), "handles_ms_median": round(h, 3), "handles_over_bank": round(h / b, 1),
            "bank_rows_per_s": round(FRAMES / (b * 1e-3)), "bank_samples_per_s": round(S * FRAMES / (b * 1e-3))}


def bank_input(cplx, seed=1):
    """(frames, S) noise, stream k scaled by 0.25 + 0.25 (k mod 8); returns the bank-layout and the stream-major device copies"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (FRAMES, S, 2 if cplx else 1)).astype(np.float32)
    x *= (0.25 + 0.25 * (np.arange(S) % 8)).astype(np.float32)[None, :, None]
    d = torch.from_numpy(x).cuda()
    return d, d.permute(1, 0, 2).contiguous()


def time_case(name, stream):
    make_bank, make_single, cplx, osz = CASES[name]
    d_bank, d_cols = bank_input(cplx)
    d_out = torch.empty(2 * S * FRAMES, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    isz = 8 if cplx else 4
    bank = make_bank()
    bank_ms = timed(stream, lambda: bank.process_dev(d_bank.data_ptr(), FRAMES, d_out.data_ptr(), stream.cuda_stream))
    bank.close()
    handles = [make_single() for _ in range(S)]

    def all_handles():
        for k, h in enumerate(handles):
            h.process_dev(d_cols.data_ptr() + k * FRAMES * isz, FRAMES, d_out.data_ptr() + k * FRAMES * osz, stream.cuda_stream)
    handles_ms = timed(stream, all_handles)
    for h in handles:
        h.close()
    return summary(bank_ms, handles_ms)


def time_channelizer_pair(stream):
    taps = dsp.windowed_sinc(16 * S, np.pi / S)
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, 2 * S * FRAMES).astype(np.float32)
    d_x = torch.from_numpy(x).cuda()
    d_ch = torch.empty((FRAMES, S, 2), dtype=torch.float32, device="cuda")
    d_out = torch.empty(S * FRAMES, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ch, bank = dsp.PolyphaseChannelizer(S, taps), dsp.BankGFSK(S, *GFSK)

    def pair():
        ch.process_dev(d_x.data_ptr(), S * FRAMES, d_ch.data_ptr(), stream.cuda_stream)
        bank.process_dev(d_ch.data_ptr(), FRAMES, d_out.data_ptr(), stream.cuda_stream)
    bank_ms = timed(stream, pair)
    bank.close()
    handles = [dsp.GFSK(*GFSK) for _ in range(S)]

    def pair_handles():
        ch.process_dev(d_x.data_ptr(), S * FRAMES, d_ch.data_ptr(), stream.cuda_stream)
        with torch.cuda.stream(stream):
            cols = d_ch.permute(1, 0, 2).contiguous()
        for k, h in enumerate(handles):
            h.process_dev(cols.data_ptr() + k * FRAMES * 8, FRAMES, d_out.data_ptr() + k * FRAMES * 4, stream.cuda_stream)
    handles_ms = timed(stream, pair_handles)
    for h in handles:
        h.close()
    return summary(bank_ms, handles_ms)


def main():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: this timing needs an MI355X"
    args = sys.argv[1:]
    out = args[0] if args and args[0].endswith(".json") else os.path.join(ROOT, "profiles", "r12", "bank_time.json")
    names = [a for a in args if not a.endswith(".json")] or list(CASES) + ["channelizer_gfsk"]
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    rec = {"streams": S, "frames": FRAMES, "timed_calls": TIMED, "cases": {}}
    if os.path.exists(out):                                     # (cases may be measured in several runs)
        with open(out) as f:
            rec["cases"] = json.load(f).get("cases", {})
    for name in names:
        r = time_channelizer_pair(stream) if name == "channelizer_gfsk" else time_case(name, stream)
        rec["cases"][name] = r
        print(f"{name}: bank {r['bank_ms_median']:.3f} ms [{min(r['bank_ms']):.3f}, {max(r['bank_ms']):.3f}], 1024 handles "
              f"{r['handles_ms_median']:.2f} ms [{min(r['handles_ms']):.2f}, {max(r['handles_ms']):.2f}], "
              f"x{r['handles_over_bank']}, {r['bank_rows_per_s'] / 1e6:.3f} M rows/s", flush=True)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    worse = [n for n, r in rec["cases"].items() if not r["bank_ms_median"] < r["handles_ms_median"]]
    assert not worse, f"banks not below their 1024-handle figure: {worse}"


if __name__ == "__main__":
    main()
