"""Call times of the symbol recovery blocks on device-resident buffers (needs an MI355X):
    python tools/time_symsync.py [out.json]        (default profiles/r11/symsync_time.json)
* the serial kernels (FastAGC, Costas<2|4|8>, MM float / complex): ms per call of 2^20 samples between
  two device events, one warm-up call and 5 timed ones (a call is tens to hundreds of ms: one
  workgroup, lane 0 walks the recurrence);
* the RDS chain: host wall time per call of 25 samples -- what one reference block of the radio module
  (1200 IF samples at 240 kS/s) leaves at 5 kS/s -- over 2000 calls after 200 warm-up calls; every call
  waits for its stream once, for MM's output count, so the wall time is the call's latency.
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


def time_serial(blk, cplx, stream):
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, 2 * N if cplx else N).astype(np.float32)
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.empty(2 * N, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    blk.process_dev(d_in.data_ptr(), N, d_out.data_ptr(), stream.cuda_stream)      # warm-up
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(TIMED):
        blk.process_dev(d_in.data_ptr(), N, d_out.data_ptr(), stream.cuda_stream)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / TIMED


def time_rds_calls(stream, n=25, warm=200, calls=2000):
    rng = np.random.default_rng(2)
    t = np.arange(n * (warm + calls)) / 5000.0
    x = (0.01 * np.sign(np.sin(2 * np.pi * 1187.5 / 2 * t)) * np.sin(2 * np.pi * 1187.5 * t) * np.exp(1j * 0.7)
         + 1e-4 * (rng.standard_normal(len(t)) + 1j * rng.standard_normal(len(t)))).astype(np.complex64)
    d_in = torch.from_numpy(x.view(np.float32)).cuda()
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = dsp.RDSBits()
    bits = 0
    for k in range(warm + calls):
        if k == warm:
            t0 = time.perf_counter()
        bits += r.process_dev(d_in.data_ptr() + 8 * n * k, n, d_out.data_ptr(), stream.cuda_stream)
    return 1e6 * (time.perf_counter() - t0) / calls, bits


def main():
    assert sdrpp_amd.lib.sdrgpu_device_count() > 0, "no HIP device visible: this timing needs an MI355X"
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11", "symsync_time.json")
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    cases = [("fast_agc_float", lambda: dsp.FastAGC(1.0, 1e6, 0.1), False),
             ("fast_agc_complex", lambda: dsp.FastAGC(1.0, 1e6, 0.1, complex_data=True), True),
             ("costas_2", lambda: dsp.Costas(2, 0.005), True), ("costas_4", lambda: dsp.Costas(4, 0.005), True),
             ("costas_8", lambda: dsp.Costas(8, 0.005), True),
             ("mm_float", lambda: dsp.MM(4.0, 2.5e-5, 0.01, 0.01), False),
             ("mm_complex", lambda: dsp.MM(4.0, 2.5e-5, 0.01, 0.01, complex_data=True), True)]
    rec = {"samples_per_call": N, "timed_calls": TIMED, "ms_per_call": {}}
    for name, make, cplx in cases:
        ms = time_serial(make(), cplx, stream)
        rec["ms_per_call"][name] = round(ms, 3)
        print(f"{name}: {ms:.3f} ms per 2^20 samples ({N / ms / 1e3:.2f} MS/s)", flush=True)
    us, bits = time_rds_calls(stream)
    rec["rds_chain"] = {"samples_per_call": 25, "calls": 2000, "us_per_call": round(us, 2), "bits_out": bits}
    print(f"rds chain: {us:.2f} us per 25-sample call", flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
