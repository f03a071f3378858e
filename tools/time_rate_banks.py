"""Call times of the rate-changing banks against the same work on single-stream handles (needs an MI355X):
    python tools/time_rate_banks.py [out.json] [case ...]     (default profiles/r17/bank_rate_time.json, every case)
The shape, the two sides and the timing of tools/time_audio_banks.py: S = 1024 streams of 1024 frames on device-resident
buffers, one bank call against 1024 single-stream handles fed their columns back to back, device events, one warm-up
call and 5 timed ones, the median with min and max. Every bank is timed in both forms of its kernel (bank_rate_kernels.h):
tiled (bank_ms) and direct (direct_ms), chosen at creation through SDRGPU_TUNING=1 SDRGPU_BANK_RATE_TILED=1 | 0.
  dfir69_d2            BankDecimatingFIR(69 taps of decim_plan(2), / 2), C64, against dsp.DecimatingFIR
  power_decimator_4    BankPowerDecimator(4) (12 taps / 2, 69 taps / 2), C64, against dsp.PowerDecimator
  polyphase_4000_4069  BankPolyphaseResampler(4000, 4069) alone with the rational resampler's taps (78 per phase), F32,
                       against dsp.PolyphaseResampler
  rational_f32 / _c64  BankRationalResampler(195312.5 -> 48000): / 4, then 4000 / 4069, against dsp.RationalResampler
  channelizer_fm_rational   sdrgpu_channelizer(1024) -> BankFM -> BankRationalResampler(F32) on device buffers; on the
                       handles side the channelizer output is transposed to stream-major first, inside the timed region
Per case also bytes in plus bytes out (of the bank: rows x S x element size, intermediate buffers not counted) over the
median time. Recorded, not tuned: a bank that is not below its handles figure is listed in the record ("not_faster")."""
import contextlib
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
from time_audio_banks import noise, timed  # noqa: E402

IN_SR, OUT_SR = 200e6 / 1024, 48000.0                            # a 1024-channel channelizer at 200 MS/s -> audio
PLAN69 = dsp.decim_plan(2)[0][1]


def rational_taps():
    """the polyphase stage of RationalResampler(195312.5 -> 48000): / 4 first, then 4000 / 4069"""
    return dsp.low_pass(OUT_SR / 2, OUT_SR / 2 * 0.1, IN_SR / 4 * 4000) * np.float32(4000)


# name: (bank(S), single-stream handle, complex data)
CASES = {
    "dfir69_d2": (lambda: dsp.BankDecimatingFIR(S, PLAN69, 2), lambda: dsp.DecimatingFIR(PLAN69, 2), True),
    "power_decimator_4": (lambda: dsp.BankPowerDecimator(S, 4), lambda: dsp.PowerDecimator(4), True),
    "polyphase_4000_4069": (lambda: dsp.BankPolyphaseResampler(S, 4000, 4069, rational_taps(), complex_data=False),
                            lambda: dsp.PolyphaseResampler(4000, 4069, rational_taps(), complex_data=False), False),
    "rational_f32": (lambda: dsp.BankRationalResampler(S, IN_SR, OUT_SR, complex_data=False),
                     lambda: dsp.RationalResampler(IN_SR, OUT_SR, complex_data=False), False),
    "rational_c64": (lambda: dsp.BankRationalResampler(S, IN_SR, OUT_SR), lambda: dsp.RationalResampler(IN_SR, OUT_SR), True),
}


@contextlib.contextmanager
def form(tiled):
    keys = ("SDRGPU_TUNING", "SDRGPU_BANK_RATE_TILED")
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update(SDRGPU_TUNING="1", SDRGPU_BANK_RATE_TILED="1" if tiled else "0")
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def record(bank_ms, direct_ms, handles_ms, bytes_moved, rows):
    r = summary(bank_ms, handles_ms)
    d = float(np.median(direct_ms))
    r.update({"direct_ms": [round(v, 4) for v in direct_ms], "direct_ms_median": round(d, 4),
              "direct_over_tiled": round(d / r["bank_ms_median"], 2), "rows_out_first_call": rows, "bytes_in_plus_out": bytes_moved,
              "gbytes_per_s": round(bytes_moved / (r["bank_ms_median"] * 1e-3) / 1e9, 1),
              "direct_gbytes_per_s": round(bytes_moved / (d * 1e-3) / 1e9, 1)})
    return r


def time_case(name, stream):
    make_bank, make_single, cplx = CASES[name]
    d_bank = torch.from_numpy(noise(cplx)).cuda()
    d_cols = d_bank.permute(1, 0, 2).contiguous()
    d_out = torch.empty(2 * S * FRAMES, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    esz = 8 if cplx else 4
    ms = {}
    for tiled in (True, False):
        with form(tiled):
            bank = make_bank()
        rows = bank.out_rows(FRAMES)
        ms[tiled] = timed(stream, lambda: bank.process_dev(d_bank.data_ptr(), FRAMES, d_out.data_ptr(), stream.cuda_stream))
        bank.close()
    handles = [make_single() for _ in range(S)]

    def all_handles():
        for k, h in enumerate(handles):
            h.process_dev(d_cols.data_ptr() + k * FRAMES * esz, FRAMES, d_out.data_ptr() + k * FRAMES * esz, stream.cuda_stream)
    handles_ms = timed(stream, all_handles)
    for h in handles:
        h.close()
    return record(ms[True], ms[False], handles_ms, (FRAMES + rows) * S * esz, rows)


def time_channelizer_fm_rational(stream):
    taps = dsp.windowed_sinc(16 * S, np.pi / S)
    rng = np.random.default_rng(2)
    d_x = torch.from_numpy(rng.uniform(-1, 1, 2 * S * FRAMES).astype(np.float32)).cuda()
    d_ch = torch.empty((FRAMES, S, 2), dtype=torch.float32, device="cuda")
    d_fm = torch.empty(S * FRAMES, dtype=torch.float32, device="cuda")
    d_out = torch.empty(S * FRAMES, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ch = dsp.PolyphaseChannelizer(S, taps)
    ms = {}
    for tiled in (True, False):
        with form(tiled):
            fm, rr = dsp.BankFM(S, IN_SR, 12500.0), dsp.BankRationalResampler(S, IN_SR, OUT_SR, complex_data=False)
        rows = rr.out_rows(FRAMES)

        def chain():
            ch.process_dev(d_x.data_ptr(), S * FRAMES, d_ch.data_ptr(), stream.cuda_stream)
            fm.process_dev(d_ch.data_ptr(), FRAMES, d_fm.data_ptr(), stream.cuda_stream)
            rr.process_dev(d_fm.data_ptr(), FRAMES, d_out.data_ptr(), stream.cuda_stream)
        ms[tiled] = timed(stream, chain)
        fm.close()
        rr.close()
    fms = [dsp.FM(IN_SR, 12500.0) for _ in range(S)]
    rrs = [dsp.RationalResampler(IN_SR, OUT_SR, complex_data=False) for _ in range(S)]

    def chain_handles():
        ch.process_dev(d_x.data_ptr(), S * FRAMES, d_ch.data_ptr(), stream.cuda_stream)
        with torch.cuda.stream(stream):
            cols = d_ch.permute(1, 0, 2).contiguous()
        for k in range(S):
            fms[k].process_dev(cols.data_ptr() + k * FRAMES * 8, FRAMES, d_fm.data_ptr() + k * FRAMES * 4, stream.cuda_stream)
            rrs[k].process_dev(d_fm.data_ptr() + k * FRAMES * 4, FRAMES, d_out.data_ptr() + k * FRAMES * 4, stream.cuda_stream)
    handles_ms = timed(stream, chain_handles)
    for h in fms + rrs:
        h.close()
    return record(ms[True], ms[False], handles_ms, S * FRAMES * 8 + rows * S * 4, rows)


def main():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: this timing needs an MI355X"
    args = sys.argv[1:]
    out = args[0] if args and args[0].endswith(".json") else os.path.join(ROOT, "profiles", "r17", "bank_rate_time.json")
    names = [a for a in args if not a.endswith(".json")] or list(CASES) + ["channelizer_fm_rational"]
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    rec = {"streams": S, "frames": FRAMES, "timed_calls": TIMED, "cases": {}}
    if os.path.exists(out):                                     # (cases may be measured in several runs)
        with open(out) as f:
            rec["cases"] = json.load(f).get("cases", {})
    for name in names:
        r = time_channelizer_fm_rational(stream) if name == "channelizer_fm_rational" else time_case(name, stream)
        rec["cases"][name] = r
        print(f"{name}: tiled {r['bank_ms_median']:.3f} ms [{min(r['bank_ms']):.3f}, {max(r['bank_ms']):.3f}] {r['gbytes_per_s']} GB/s, "
              f"direct {r['direct_ms_median']:.3f} ms [{min(r['direct_ms']):.3f}, {max(r['direct_ms']):.3f}] {r['direct_gbytes_per_s']} GB/s, "
              f"1024 handles {r['handles_ms_median']:.2f} ms [{min(r['handles_ms']):.2f}, {max(r['handles_ms']):.2f}], "
              f"x{r['handles_over_bank']}", flush=True)
        rec["not_faster"] = [n for n, c in rec["cases"].items()
                             if not max(c["bank_ms_median"], c["direct_ms_median"]) < c["handles_ms_median"]]
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
