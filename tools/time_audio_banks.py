"""Call times of the analogue receiver banks against the same work on single-stream handles (needs an MI355X):
    python tools/time_audio_banks.py [out.json] [case ...]     (default profiles/r13/bank_audio_time.json, every case)
The shape, the two sides and the timing of tools/time_banks.py: S = 1024 streams of 1024 frames on
device-resident buffers, one bank call against 1024 single-stream handles fed their columns back to back, device
events, one warm-up call and 5 timed ones, the median with min and max.
The AGC is timed twice: on noise that never clips (initial gain 1: the running amplitude starts at the set
point), and on a bursty signal (level steps over 60 dB, x50 spikes) with AM's parameters and a reset before
every call, outside the timed region, so that every call starts from the initial gain of infinity and the
clip look-ahead fires in every stream. Both sides of a case get the same treatment.
The channelizer pair times sdrgpu_channelizer(1024) -> BankSquelch -> BankFM on its device output; on the
handles side the channelizer output is transposed to stream-major first, inside the timed region.
Recorded, not tuned: a bank that is not below its handles figure is listed in the record ("not_faster")."""
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

FS = 48000.0
AGC = (1.0, 50.0 / FS, 5.0 / FS, 10e6, 10.0)
AM = (10000.0, 50.0 / FS, 5.0 / FS, 10.0 / FS, FS)
INF = float("inf")


def noise(cplx, seed=1):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (FRAMES, S, 2 if cplx else 1)).astype(np.float32)
    return x * (0.25 + 0.25 * (np.arange(S) % 8)).astype(np.float32)[None, :, None]


def bursty(cplx, seed=3):
    """magnitude 0.5..1 times level steps of 26, 8 and 26 dB over the call, x50 spikes at rows 32a, 32a + 31 and
    32a + (k mod 32) for four a, a run of zeros: the signal of tests/_bank_audio.py at this shape"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 1.0, (FRAMES, S, 2 if cplx else 1)) * rng.choice([-1.0, 1.0], (FRAMES, S, 2 if cplx else 1))
    level = np.repeat([1e-3, 2e-2, 5e-2, 1.0], FRAMES // 4)
    x *= level[:, None, None]
    k = np.arange(S)
    for a in (3, 12, 20, 29):
        for rows in (np.full(S, 32 * a), np.full(S, 32 * a + 31), 32 * a + k % 32):
            x[rows, k, :] = 50.0 * level[rows][:, None]
    x[100:140] = 0
    return x.astype(np.float32)


def limiter(cplx):
    a = dsp.AGC(*AGC, 3.5, complex_data=cplx)
    a.set_enabled(False)
    a.set_gain(3.5)
    return a


# name: (bank(S), single-stream handle, complex input, bytes per output element, input, reset before every call)
CASES = {
    "agc_float_noise": (lambda: dsp.BankAGC(S, *AGC, 1.0), lambda: dsp.AGC(*AGC, 1.0), False, 4, noise, False),
    "agc_complex_noise": (lambda: dsp.BankAGC(S, *AGC, 1.0, complex_data=True), lambda: dsp.AGC(*AGC, 1.0, complex_data=True), True, 8,
                          noise, False),
    "agc_float_bursty": (lambda: dsp.BankAGC(S, *AGC, INF), lambda: dsp.AGC(*AGC, INF), False, 4, bursty, True),
    "agc_complex_bursty": (lambda: dsp.BankAGC(S, *AGC, INF, complex_data=True), lambda: dsp.AGC(*AGC, INF, complex_data=True), True, 8,
                           bursty, True),
    "agc_limiter_complex": (lambda: dsp.BankAGC(S, *AGC, 3.5, complex_data=True, enabled=False), lambda: limiter(True), True, 8, noise,
                            False),
    "dc_blocker_float": (lambda: dsp.BankDCBlocker(S, 10.0 / FS), lambda: dsp.DCBlocker(10.0 / FS), False, 4, noise, False),
    "dc_blocker_complex": (lambda: dsp.BankDCBlocker(S, 10.0 / FS, complex_data=True), lambda: dsp.DCBlocker(10.0 / FS, True), True, 8,
                           noise, False),
    "deemphasis": (lambda: dsp.BankDeemphasis(S, 50e-6, FS), lambda: dsp.Deemphasis(50e-6, FS), False, 4, noise, False),
    "squelch": (lambda: dsp.BankSquelch(S, -8.0), lambda: dsp.Squelch(-8.0), True, 8, noise, False),
    "fm": (lambda: dsp.BankFM(S, FS, 12500.0), lambda: dsp.FM(FS, 12500.0), True, 4, noise, False),
    "am_carrier": (lambda: dsp.BankAM(S, 1, *AM), lambda: dsp.AM(1, *AM), True, 4, noise, False),
    "am_audio": (lambda: dsp.BankAM(S, 2, *AM), lambda: dsp.AM(2, *AM), True, 4, noise, False),
}


def timed(stream, call, prepare=None):
    ms = []
    for i in range(TIMED + 1):                                   # the first call is the warm-up
        if prepare:
            prepare()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms[1:]


def time_case(name, stream):
    make_bank, make_single, cplx, osz, make_input, resets = CASES[name]
    d_bank = torch.from_numpy(make_input(cplx)).cuda()
    d_cols = d_bank.permute(1, 0, 2).contiguous()
    d_out = torch.empty(2 * S * FRAMES, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    isz = 8 if cplx else 4
    bank = make_bank()
    bank_ms = timed(stream, lambda: bank.process_dev(d_bank.data_ptr(), FRAMES, d_out.data_ptr(), stream.cuda_stream),
                    bank.reset if resets else None)
    bank.close()
    handles = [make_single() for _ in range(S)]

    def all_handles():
        for k, h in enumerate(handles):
            h.process_dev(d_cols.data_ptr() + k * FRAMES * isz, FRAMES, d_out.data_ptr() + k * FRAMES * osz, stream.cuda_stream)

    def reset_handles():
        for h in handles:
            h.reset()
    handles_ms = timed(stream, all_handles, reset_handles if resets else None)
    for h in handles:
        h.close()
    return summary(bank_ms, handles_ms)


def time_channelizer_pair(stream):
    taps = dsp.windowed_sinc(16 * S, np.pi / S)
    rng = np.random.default_rng(2)
    d_x = torch.from_numpy(rng.uniform(-1, 1, 2 * S * FRAMES).astype(np.float32)).cuda()
    d_ch = torch.empty((FRAMES, S, 2), dtype=torch.float32, device="cuda")
    d_sq = torch.empty((FRAMES, S, 2), dtype=torch.float32, device="cuda")
    d_out = torch.empty(S * FRAMES, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ch, sq, fm = dsp.PolyphaseChannelizer(S, taps), dsp.BankSquelch(S, -60.0), dsp.BankFM(S, FS, 12500.0)

    def pair():
        ch.process_dev(d_x.data_ptr(), S * FRAMES, d_ch.data_ptr(), stream.cuda_stream)
        sq.process_dev(d_ch.data_ptr(), FRAMES, d_sq.data_ptr(), stream.cuda_stream)
        fm.process_dev(d_sq.data_ptr(), FRAMES, d_out.data_ptr(), stream.cuda_stream)
    bank_ms = timed(stream, pair)
    sq.close()
    fm.close()
    sqs, fms = [dsp.Squelch(-60.0) for _ in range(S)], [dsp.FM(FS, 12500.0) for _ in range(S)]

    def pair_handles():
        ch.process_dev(d_x.data_ptr(), S * FRAMES, d_ch.data_ptr(), stream.cuda_stream)
        with torch.cuda.stream(stream):
            cols = d_ch.permute(1, 0, 2).contiguous()
        for k in range(S):
            sqs[k].process_dev(cols.data_ptr() + k * FRAMES * 8, FRAMES, d_sq.data_ptr() + k * FRAMES * 8, stream.cuda_stream)
            fms[k].process_dev(d_sq.data_ptr() + k * FRAMES * 8, FRAMES, d_out.data_ptr() + k * FRAMES * 4, stream.cuda_stream)
    handles_ms = timed(stream, pair_handles)
    for h in sqs + fms:
        h.close()
    return summary(bank_ms, handles_ms)


def main():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: this timing needs an MI355X"
    args = sys.argv[1:]
    out = args[0] if args and args[0].endswith(".json") else os.path.join(ROOT, "profiles", "r13", "bank_audio_time.json")
    names = [a for a in args if not a.endswith(".json")] or list(CASES) + ["channelizer_squelch_fm"]
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    rec = {"streams": S, "frames": FRAMES, "timed_calls": TIMED, "cases": {}}
    if os.path.exists(out):                                     # (cases may be measured in several runs)
        with open(out) as f:
            rec["cases"] = json.load(f).get("cases", {})
    for name in names:
        r = time_channelizer_pair(stream) if name == "channelizer_squelch_fm" else time_case(name, stream)
        rec["cases"][name] = r
        print(f"{name}: bank {r['bank_ms_median']:.3f} ms [{min(r['bank_ms']):.3f}, {max(r['bank_ms']):.3f}], 1024 handles "
              f"{r['handles_ms_median']:.2f} ms [{min(r['handles_ms']):.2f}, {max(r['handles_ms']):.2f}], "
              f"x{r['handles_over_bank']}, {r['bank_rows_per_s'] / 1e6:.3f} M rows/s", flush=True)
        rec["not_faster"] = [n for n, c in rec["cases"].items() if not c["bank_ms_median"] < c["handles_ms_median"]]
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
