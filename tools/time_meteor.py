"""Call times of the carrier loops and the Meteor demodulator on device-resident buffers (needs an MI355X):
    python tools/time_meteor.py [out.json]        (default profiles/r21/meteor_time.json)
* the serial kernels (PLL, CarrierPLL, MeteorCostas plain / broken modulation): ms per call of 2^20 samples between two
  device events, one warm-up call and 5 timed ones (one workgroup, lane 0 walks the recurrence, as for Costas);
* the Meteor composite (main.cpp:66's parameters, OQPSK on): host wall time per call of a 150 kS/s block -- 15000
  samples, 100 ms of the module's input -- over 200 calls after 20 warm-up calls; every call waits for its stream once,
  for MM's output count, so the wall time is the call's latency;
* the banks at S = 1024 streams of 1024 frames: ms per call between two device events (BankMeteor: wall time, it waits
  for its counts), one warm-up call and 5 timed ones, the median with min and max.
Recorded, not tuned: there is no bar on these."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdrpp_amd  # noqa: E402
from sdrpp_amd import dsp  # noqa: E402

N = 1 << 20
TIMED = 5
S, FRAMES = 1024, 1024
BLOCK = 15000
METEOR = (72000.0, 150000.0, 33, 0.6, 0.1, 0.005, False, True, 1e-6, 0.01, 0.01)


def noise(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, 2 * n).astype(np.float32)).cuda()


def time_serial(blk, stream):
    d_in, d_out = noise(N, 1), torch.empty(2 * N, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    blk.process_dev(d_in.data_ptr(), N, d_out.data_ptr(), stream.cuda_stream)      # warm-up
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(TIMED):
        blk.process_dev(d_in.data_ptr(), N, d_out.data_ptr(), stream.cuda_stream)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / TIMED


def time_meteor_calls(stream, warm=20, calls=200):
    d_in, d_out = noise(BLOCK * 8, 2), torch.empty(2 * BLOCK, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    m = dsp.Meteor(*METEOR)
    symbols = 0
    for k in range(warm + calls):
        if k == warm:
            t0 = time.perf_counter()
        symbols += m.process_dev(d_in.data_ptr() + 8 * BLOCK * (k % 8), BLOCK, d_out.data_ptr(), stream.cuda_stream)
    return 1e3 * (time.perf_counter() - t0) / calls, symbols


def time_bank(bank, stream, waits):
    d_in, d_out = noise(S * FRAMES, 3), torch.empty(2 * S * FRAMES, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    call = lambda: bank.process_dev(d_in.data_ptr(), FRAMES, d_out.data_ptr(), stream.cuda_stream)
    call()                                                       # warm-up
    stream.synchronize()
    ms = []
    for _ in range(TIMED):
        if waits:
            t0 = time.perf_counter()
            call()
            ms.append(1e3 * (time.perf_counter() - t0))
        else:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    bank.close()
    return {"ms": [round(v, 4) for v in ms], "ms_median": round(float(np.median(ms)), 4),
            "samples_per_s": round(S * FRAMES / (float(np.median(ms)) * 1e-3))}


def main():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: this timing needs an MI355X"
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r21", "meteor_time.json")
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    rec = {"samples_per_call": N, "timed_calls": TIMED, "ms_per_call": {}}
    for name, make in [("pll", lambda: dsp.PLL(0.01)), ("carrier_pll", lambda: dsp.CarrierPLL(0.01)),
                       ("meteor_costas", lambda: dsp.MeteorCostas(0.005, False)),
                       ("meteor_costas_broken", lambda: dsp.MeteorCostas(0.005, True))]:
        ms = time_serial(make(), stream)
        rec["ms_per_call"][name] = round(ms, 3)
        print(f"{name}: {ms:.3f} ms per 2^20 samples ({N / ms / 1e3:.2f} MS/s)", flush=True)
    ms, symbols = time_meteor_calls(stream)
    rec["meteor"] = {"samples_per_call": BLOCK, "calls": 200, "ms_per_call": round(ms, 4), "symbols_out": symbols,
                     "input_ms_per_call": 1e3 * BLOCK / 150000.0}
    print(f"meteor: {ms:.3f} ms per {BLOCK}-sample call (100 ms of input at 150 kS/s)", flush=True)
    rec["banks"] = {"streams": S, "frames": FRAMES, "cases": {}}
    for name, make, waits in [("pll", lambda: dsp.BankPLL(S, 0.01), False), ("carrier_pll", lambda: dsp.BankCarrierPLL(S, 0.01), False),
                              ("meteor_costas", lambda: dsp.BankMeteorCostas(S, 0.005, False), False),
                              ("meteor_costas_broken", lambda: dsp.BankMeteorCostas(S, 0.005, True), False),
                              ("meteor", lambda: dsp.BankMeteor(S, *METEOR), True)]:
        r = time_bank(make(), stream, waits)
        rec["banks"]["cases"][name] = r
        print(f"bank {name}: {r['ms_median']:.3f} ms [{min(r['ms']):.3f}, {max(r['ms']):.3f}], {r['samples_per_s'] / 1e6:.1f} MS/s", flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
