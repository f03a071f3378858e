"""Call times of the SSB and CW receiver banks against the same work on single-stream handles (needs an MI355X):
    python tools/time_ssb_banks.py [out.json] [case ...]     (default profiles/r14/bank_ssb_time.json, every case)
The shape, the two sides and the timing of tools/time_audio_banks.py (whose time_case runs the cases here): S = 1024
streams of 1024 frames on device-resident buffers, one bank call against 1024 single-stream handles fed their columns
back to back, device events, one warm-up call and 5 timed ones, the median with min and max.
  xlator, xlate_real   BankXlator and its real-part form against 1024 dsp.FrequencyXlator handles (which write complex
                       samples: the single-stream route has no translate-and-take-real block)
  ssb_agc_on / _off    BankSSB (USB) against 1024 dsp.SSB handles, on noise
  cw_noise             BankCW against 1024 dsp.CW handles on noise of 0.25..2 per stream: with CW's AGC (max output 1,
                       initial gain 1) the clip look-ahead fires whenever a sample rises above the running amplitude
  agc_float_cw         the AGC stage of BankCW alone (BankAGC<F32> with CW's constants) on the same noise, for the
                       comparison with agc_float_noise of profiles/r13 (the same bank on noise that never clips)
  channelizer_ssb      sdrgpu_channelizer(1024) -> BankSSB on its device output; on the handles side the channelizer
                       output is transposed to stream-major first, inside the timed region
Recorded, not tuned: a bank that is not below its handles figure is listed in the record ("not_faster"); "ssb_vs_stages"
is BankSSB's median over the sum of the medians of xlate_real and of the AGC bank it runs."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdrpp_amd  # noqa: E402
from sdrpp_amd import dsp  # noqa: E402
from time_banks import S, FRAMES, TIMED, summary  # noqa: E402
import time_audio_banks as tab  # noqa: E402

FS = 24000.0
BW, TONE = 2800.0, 800.0
ATT, DEC = 50.0 / FS, 5.0 / FS
W = 2.0 * np.pi * (BW / 2.0 / FS)
SSB_AGC = (1.0, ATT, DEC, 10e6, 10.0, float("inf"))
CW_AGC = (1.0, ATT, DEC, 10e6, 1.0, 1.0)

# name: (bank(S), single-stream handle, complex input, bytes per output element, input, reset before every call)
CASES = {
    "xlator": (lambda: dsp.BankXlator(S, W), lambda: dsp.FrequencyXlator(W), True, 8, tab.noise, False),
    "xlate_real": (lambda: dsp.BankXlator(S, W, real=True), lambda: dsp.FrequencyXlator(W), True, 8, tab.noise, False),
    "ssb_agc_on": (lambda: dsp.BankSSB(S, 0, BW, FS, True, ATT, DEC), lambda: dsp.SSB(0, BW, FS, True, ATT, DEC), True, 4, tab.noise, False),
    "ssb_agc_off": (lambda: dsp.BankSSB(S, 0, BW, FS, False, ATT, DEC), lambda: dsp.SSB(0, BW, FS, False, ATT, DEC), True, 4, tab.noise,
                    False),
    "cw_noise": (lambda: dsp.BankCW(S, TONE, True, ATT, DEC, FS), lambda: dsp.CW(TONE, True, ATT, DEC, FS), True, 4, tab.noise, False),
    "agc_float_ssb": (lambda: dsp.BankAGC(S, *SSB_AGC), lambda: dsp.AGC(*SSB_AGC), False, 4, tab.noise, False),
    "agc_float_cw": (lambda: dsp.BankAGC(S, *CW_AGC), lambda: dsp.AGC(*CW_AGC), False, 4, tab.noise, False),
}
tab.CASES.update(CASES)


def time_channelizer_ssb(stream):
    taps = dsp.windowed_sinc(16 * S, np.pi / S)
    rng = np.random.default_rng(2)
    d_x = torch.from_numpy(rng.uniform(-1, 1, 2 * S * FRAMES).astype(np.float32)).cuda()
    d_ch = torch.empty((FRAMES, S, 2), dtype=torch.float32, device="cuda")
    d_out = torch.empty(S * FRAMES, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ch, ssb = dsp.PolyphaseChannelizer(S, taps), dsp.BankSSB(S, 0, BW, FS, True, ATT, DEC)

    def pair():
        ch.process_dev(d_x.data_ptr(), S * FRAMES, d_ch.data_ptr(), stream.cuda_stream)
        ssb.process_dev(d_ch.data_ptr(), FRAMES, d_out.data_ptr(), stream.cuda_stream)
    bank_ms = tab.timed(stream, pair)
    ssb.close()
    hs = [dsp.SSB(0, BW, FS, True, ATT, DEC) for _ in range(S)]

    def pair_handles():
        ch.process_dev(d_x.data_ptr(), S * FRAMES, d_ch.data_ptr(), stream.cuda_stream)
        with torch.cuda.stream(stream):
            cols = d_ch.permute(1, 0, 2).contiguous()
        for k in range(S):
            hs[k].process_dev(cols.data_ptr() + k * FRAMES * 8, FRAMES, d_out.data_ptr() + k * FRAMES * 4, stream.cuda_stream)
    handles_ms = tab.timed(stream, pair_handles)
    for h in hs:
        h.close()
    return summary(bank_ms, handles_ms)


def main():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: this timing needs an MI355X"
    args = sys.argv[1:]
    out = args[0] if args and args[0].endswith(".json") else os.path.join(ROOT, "profiles", "r14", "bank_ssb_time.json")
    names = [a for a in args if not a.endswith(".json")] or list(CASES) + ["channelizer_ssb"]
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    rec = {"streams": S, "frames": FRAMES, "timed_calls": TIMED, "cases": {}}
    if os.path.exists(out):                                     # (cases may be measured in several runs)
        with open(out) as f:
            rec["cases"] = json.load(f).get("cases", {})
    for name in names:
        r = time_channelizer_ssb(stream) if name == "channelizer_ssb" else tab.time_case(name, stream)
        rec["cases"][name] = r
        print(f"{name}: bank {r['bank_ms_median']:.3f} ms [{min(r['bank_ms']):.3f}, {max(r['bank_ms']):.3f}], 1024 handles "
              f"{r['handles_ms_median']:.2f} ms [{min(r['handles_ms']):.2f}, {max(r['handles_ms']):.2f}], "
              f"x{r['handles_over_bank']}, {r['bank_rows_per_s'] / 1e6:.3f} M rows/s", flush=True)
        c = rec["cases"]
        rec["not_faster"] = [n for n, v in c.items() if not v["bank_ms_median"] < v["handles_ms_median"]]
        if all(n in c for n in ("ssb_agc_on", "xlate_real", "agc_float_ssb")):
            rec["ssb_vs_stages"] = round(c["ssb_agc_on"]["bank_ms_median"] / (c["xlate_real"]["bank_ms_median"] + c["agc_float_ssb"]["bank_ms_median"]), 3)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
